// pv_lock.hpp — identity phase locking of one STANDARD frame (Laroche & Dolson; DESIGN.md
// §3.6): the peaks of the frame's magnitude row and, for every bin, the phase offset of the
// peak that owns it.  Used by synth_frame's locked mode (pv_frame.hpp) in k_synthesis in
// the locked mode (pv_syn_kernel.hpp, instantiated in pv_locked.hip).
#pragma once
#include "pv_device.hpp"

namespace pv {

// synth_frame / syn_run MODE of the locked STANDARD time stretch
constexpr int kModeLocked = 6;
// ... and of the stretch with the transient phase reset (pv_transient.hpp), unlocked and locked
constexpr int kModeReset = 10;
constexpr int kModeLockedReset = 11;
// ... and of the time-map stretch (pv_timemap.hpp), unlocked and locked
constexpr int kModeMap = 12;
constexpr int kModeLockedMap = 13;

// A wave holds the frame: bin k = lane + 64 i in register slot i (i < E), bin L = 64 E in slot
// E of lane 0.  Slot E of the other lanes stands for the bins past L, which do not exist: they
// carry -inf, so they are never peaks and never stop a neighbour from being one.
//
// Peaks (bin k is one iff mag[k] > mag[k'] strictly for k' = k-2, k-1, k+1, k+2 inside
// [0, L]): the upper neighbours k+1, k+2 come from lanes +1, +2 of the same slot (the last
// lanes take them from slot i+1 of lanes 0, 1: the source lanes offer that slot) by
// ds_bpermute, crossbar only.  The four comparisons "k > k+d" and "k+d > k" are ballots,
// wave-uniform 64-bit words; "k > k-d" is the word "k+d > k" shifted up by d bits across the
// slot words, so the lower neighbours need no exchange of their own.  A NaN compares false
// both ways: it is no peak and neither are the bins next to it.
//
// Owner (the nearest peak, the lower one on a tie; the bin itself if the frame has none):
// the nearest peak at or below k and the nearest above it are find-last / find-first bit of
// the slot's peak word masked at the lane, or the wave-uniform nearest peak of the slot words
// below / above.
//
// theta[i] (the slot's output-minus-analysis phase in revolutions) goes to th[k] (LDS, L + 2
// floats: th[L + 1] takes the other lanes' slot E) and comes back as own[i] = theta[owner]:
// one LDS round trip per bin.
template <int L>
__device__ __forceinline__ void lock_offsets(const float (&mag)[L / 64 + 1], const float (&theta)[L / 64 + 1],
                                             int lane, float* th, float (&own)[L / 64 + 1]) {
    constexpr int E = L / 64;
    constexpr int kNone = 1 << 20;  // farther than any bin
    typedef unsigned long long u64;
    const float ninf = -__builtin_inff();
    const int up1 = ((lane + 1) & 63) << 2, up2 = ((lane + 2) & 63) << 2;
    u64 g1[E + 1], g2[E + 1], u1[E + 1], u2[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        const float m = (i < E) ? mag[i] : (lane == 0 ? mag[E] : ninf);
        const float mn = (i + 1 < E) ? mag[(i + 1 < E) ? i + 1 : 0] : (i + 1 == E && lane == 0) ? mag[E] : ninf;
        const float n1 = __int_as_float(__builtin_amdgcn_ds_bpermute(up1, __float_as_int(lane < 1 ? mn : m)));
        const float n2 = __int_as_float(__builtin_amdgcn_ds_bpermute(up2, __float_as_int(lane < 2 ? mn : m)));
        g1[i] = __builtin_amdgcn_ballot_w64(m > n1);
        u1[i] = __builtin_amdgcn_ballot_w64(n1 > m);
        g2[i] = __builtin_amdgcn_ballot_w64(m > n2);
        u2[i] = __builtin_amdgcn_ballot_w64(n2 > m);
    }
    u64 pk[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        // bins 0 and 1 have no neighbour below 0: those comparisons count as won
        const u64 d1 = (u1[i] << 1) | (i > 0 ? u1[i > 0 ? i - 1 : 0] >> 63 : 1ull);
        const u64 d2 = (u2[i] << 2) | (i > 0 ? u2[i > 0 ? i - 1 : 0] >> 62 : 3ull);
        pk[i] = g1[i] & g2[i] & d1 & d2;
    }
    // nearest peak in the slot words below / above (wave-uniform)
    int below[E + 1], above[E + 1];
    int run = -kNone;
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        below[i] = run;
        if (pk[i]) run = 64 * i + 63 - __builtin_clzll(pk[i]);
    }
    const bool any = run != -kNone;
    run = kNone;
#pragma unroll
    for (int i = E; i >= 0; --i) {
        above[i] = run;
        if (pk[i]) run = 64 * i + __builtin_ctzll(pk[i]);
    }
#pragma unroll
    for (int i = 0; i < E; ++i) th[lane + 64 * i] = theta[i];
    th[lane == 0 ? L : L + 1] = theta[E];
    wave_lds_sync();
    const u64 le = (2ull << lane) - 1ull;  // bits 0 .. lane
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        // (slot E: bin L on every lane; only lane 0 uses it, the others stay in range)
        const int k = (i < E) ? lane + 64 * i : L;
        const u64 mle = (i < E) ? le : 1ull;
        const u64 lo_w = pk[i] & mle, hi_w = pk[i] & ~mle;
        const int lo = lo_w ? 64 * i + 63 - __builtin_clzll(lo_w) : below[i];
        const int hi = hi_w ? 64 * i + __builtin_ctzll(hi_w) : above[i];
        int o = (k - lo <= hi - k) ? lo : hi;
        o = any ? o : k;
        own[i] = lds_ld(&th[o]);
    }
}

}  // namespace pv
