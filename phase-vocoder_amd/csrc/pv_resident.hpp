// pv_resident.hpp — the two frame bodies of the channel-resident STANDARD time stretch
// (k_resident, pv_resident.hip): one analysis frame whose {mag, phase} row goes to LDS, and the
// LDS carve-up the roles share.  The analysis frame is k_std_analysis's (pv_ana_run.hpp: fft_run,
// bin_l_real and the mirrored-pair split of ana_run's PAIR branch, copied here without its
// decisions, records and global stores: factored out of ana_run it would have to leave that
// kernel's assembly unchanged), so a row holds the bits that kernel writes to the spectrum; the
// synthesis side calls synth_frame, ola_add and ola_shift itself.
#pragma once
#include "pv_frame.hpp"
#include "pv_kernels.h"

namespace pv {

constexpr int kResWaves = 3;  // waves per workgroup: two analysis waves, one synthesis wave
constexpr int kResRing = 4;   // rows in flight: the pair being written and the pair being read

// LDS of one workgroup, in float2 units: stage-major twiddles, split twiddles, a tile per wave
// and the row ring.  L = 512: 38 336 bytes, four workgroups per CU.
template <int L>
struct ResGeo {
    static constexpr int ROW = L + 2;  // bins 0 .. L (+1 pad: rows stay 16-byte aligned)
    static constexpr int O_TW = 0;
    static constexpr int O_TWS = O_TW + L;
    static constexpr int O_TILE = O_TWS + (L + 2);
    static constexpr int O_RING = O_TILE + kResWaves * Geo<L>::TILE;
    static constexpr int SIZE = O_RING + kResRing * ROW;
    static constexpr size_t BYTES = sizeof(float2) * SIZE;
    static_assert(O_TILE % 2 == 0 && O_RING % 2 == 0 && ROW % 2 == 0, "16-byte alignment of the carve-up");
};

// Shifted input of an analysis wave.  A wave takes every second frame, so from one of its frames
// to the next the input advances two hops of N / 4: N / 2 samples, D = E / 2 of the E sample
// pairs a lane holds.  Only the D new pairs are loaded, and no register is moved: the wave walks
// its frames in groups of RR = E / D = 2, and the frame of rotation phase r holds its logical
// pair q (samples 2 (lane + 64 q) + {0, 1} from the frame's start) in physical register
// res_rot_reg (ana_run's window_rot with D = 4, RR = 2).
template <int E>
struct ResRot {
    static constexpr int D = E / 2;
    static constexpr int RR = 2;
    static constexpr int reg(int q, int r) { return (q + D * r) % E; }
    // the wave's next frame after a frame of phase r has phase (r + 1) mod RR; its logical pair
    // q < E - D is this frame's pair q + D and must already sit in the register the map names
    static constexpr bool kept_in_place() {
        for (int r = 0; r < RR; ++r)
            for (int q = 0; q < E - D; ++q)
                if (reg(q, (r + 1) % RR) != reg(q + D, r)) return false;
        return true;
    }
    // its new pairs q >= E - D land only in registers whose pairs (q < D) this frame's window
    // multiply has consumed, never in one that holds a pair the next frame keeps
    static constexpr bool new_in_free() {
        for (int r = 0; r < RR; ++r)
            for (int q = E - D; q < E; ++q) {
                const int dst = reg(q, (r + 1) % RR);
                bool freed = false;
                for (int k = 0; k < D; ++k) freed = freed || reg(k, r) == dst;
                if (!freed) return false;
                for (int k = D; k < E; ++k)
                    if (reg(k, r) == dst) return false;
            }
        return true;
    }
    // every phase's map is a permutation of the E registers
    static constexpr bool one_to_one() {
        for (int r = 0; r < RR; ++r)
            for (int q = 0; q < E; ++q)
                for (int k = 0; k < q; ++k)
                    if (reg(k, r) == reg(q, r)) return false;
        return true;
    }
    static_assert(E % 2 == 0 && RR * D == E, "two frames move the window by E registers");
    static_assert(one_to_one(), "a phase's pairs sit in E different registers");
    static_assert(kept_in_place(), "the pairs a frame keeps for the next one are where its map reads them");
    static_assert(new_in_free(), "new pairs overwrite only pairs the frame has consumed");
};

// The waves of a workgroup meet here.  Only LDS traffic has to be complete: the rows travel
// through LDS alone, so a wave's global loads and stores stay in flight across the barrier.
__device__ __forceinline__ void res_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One analysis frame from its windowed samples z: the row of bins 0 .. L in natural order.
// Mirrored pairs, as ana_run's PAIR branch: pair i of lane l is bin k = l + 64 i (i < E / 2) and
// bin L - k, whose split operands are the same A = Z[k], B = Z[L - k] swapped: er, or are the
// same sums, ei, oi the negated differences (exact), so both bins come from one permute and one
// set of terms — bit for bit the per-bin formula (contract v2).  Lane 0's partners are bins
// 64 (E - i), and its pair 0 is (bin 0, bin L / 2), bin L / 2 being the one bin that is its own
// mirror: its operands (Z[L/2] twice) come in by a lane-0 select.  The row is in LDS, so both
// bins are written where they belong (the global rows' aligned-block store order is not needed).
template <int L>
__device__ __forceinline__ void res_ana_frame(float2 (&z)[Geo<L>::E], float2* tile, const float2* twl,
                                              const float2* twsl, const float2 (&tw0)[Geo<L>::E], int lane,
                                              float2* row) {
    constexpr int E = Geo<L>::E;
    constexpr int H = E / 2;
    fft_run<L, false, false>(z, tile, twl, tw0, lane);
    float magL, phL;
    bin_l_real<L, true>(z, twsl, magL, phL);
    const int rev = ((64 - lane) & 63) << 2;            // lane reversal l -> (64 - l) mod 64
    const float2* baseT = twsl + lane;                  // split twiddles of the lane's bins
    const int offP = L - lane;                          // partner bins L - lane - 64 i
    const int offP0 = (lane == 0) ? L / 2 : L - lane;   // pair 0's partner (lane 0: bin L/2)
    static_for<0, H>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float2 A = z[slot_reg<L>(i)];
        const float2 o = z[slot_reg<L>(E - 1 - i)];
        const float2 m = z[slot_reg<L>((E - i) & (E - 1))];
        float2 Bz;
        Bz.x = __int_as_float(__builtin_amdgcn_ds_bpermute(rev, __float_as_int(o.x)));
        Bz.y = __int_as_float(__builtin_amdgcn_ds_bpermute(rev, __float_as_int(o.y)));
        lane0_mov2(Bz.x, Bz.y, m.x, m.y);  // lane 0 read itself: its partner is m
        const int kp = (i == 0) ? offP0 : offP - 64 * i;  // the partner bin
        const float2 tw = lds_ld(&baseT[64 * i]);
        const float2 twp = lds_ld(&twsl[kp]);
        const float er = A.x + Bz.x, ei = A.y - Bz.y, orr = A.y + Bz.y, oi = Bz.x - A.x;
        float Xr = __builtin_fmaf(orr, tw.x, __builtin_fmaf(-oi, tw.y, er));  // contract v2
        float Xi = __builtin_fmaf(orr, tw.y, __builtin_fmaf(oi, tw.x, ei));
        float Xrp, Xip;
        if constexpr (i == 0) {
            if (lane == 0) Xi = 0.0f;  // bin 0 is real
            // the partner's own operands (B, A), on lane 0 (Z[L/2], Z[L/2])
            const float2 h = z[slot_reg<L>(H)];
            const bool l0 = lane == 0;
            const float ax = l0 ? h.x : Bz.x, ay = l0 ? h.y : Bz.y;
            const float bx = l0 ? h.x : A.x, by = l0 ? h.y : A.y;
            const float erp = ax + bx, eip = ay - by, orp = ay + by, oip = bx - ax;
            Xrp = __builtin_fmaf(orp, twp.x, __builtin_fmaf(-oip, twp.y, erp));
            Xip = __builtin_fmaf(orp, twp.y, __builtin_fmaf(oip, twp.x, eip));
        } else {
            // partner terms (er, -ei, or, -oi)
            Xrp = __builtin_fmaf(orr, twp.x, __builtin_fmaf(oi, twp.y, er));
            Xip = __builtin_fmaf(orr, twp.y, __builtin_fmaf(-oi, twp.x, -ei));
        }
        const f2v ph2 = atan2_pv2(Xi, Xr, Xip, Xrp);
        const float mag = half_sqrt(__builtin_fmaf(Xr, Xr, Xi * Xi));
        const float magp = half_sqrt(__builtin_fmaf(Xrp, Xrp, Xip * Xip));
        row[lane + 64 * i] = make_float2(mag, ph2.x);
        row[kp] = make_float2(magp, ph2.y);
    });
    if (lane == 0) row[L] = make_float2(magL, phL);
    wave_lds_sync();
}

}  // namespace pv
