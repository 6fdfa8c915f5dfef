// pv_warp.hpp — formant preservation of the stretch-and-resample pitch shift
// (pv_pitch_set_formant): the envelope warp of one STANDARD time-stretch
// frame.  The frame's log envelope le[k] (k_envelope, pv_formant.hip) is read at the position
// the resampler will move bin k to, k out_hop / hop, and the bin's magnitude is scaled by
//   exp(lw[k] - le[k]),  lw[k] = le[i_k] + f_k (le[min(i_k + 1, L)] - le[i_k]),
// so that after the P:Q resampling the envelope lies where the input had it.  The map
// {i_k, f_k} is the host's (pvtab::warp_map).  Used by synth_frame's warp modes (pv_frame.hpp)
// in k_synthesis in the warp modes (pv_syn_kernel.hpp, instantiated in pv_warp.hip).
#pragma once
#include "pv_device.hpp"
#include "pv_formant.hpp"
#include "pv_lock.hpp"

namespace pv {

// synth_frame / syn_run MODEs of the STANDARD time stretch with the envelope warp: the plain
// stretch (MODE 0) and the locked one (kModeLocked), each with the warp gain on its magnitudes
constexpr int kModeWarp = 8;
constexpr int kModeLockedWarp = 9;
constexpr bool mode_is_warp(int mode) { return mode == kModeWarp || mode == kModeLockedWarp; }
constexpr bool mode_is_locked(int mode) {
    return mode == kModeLocked || mode == kModeLockedWarp || mode == kModeLockedReset;
}

// A wave holds the frame: bin k = lane + 64 i in register slot i (i < E), bin L in slot E
// (every lane holds le[L]; lane 0's is the one that counts).  le goes to wt[k] (LDS, L + 2
// floats: wt[L + 1] takes the other lanes' slot E), every bin reads its map entry {i_k, bits of
// f_k} (wmap, LDS, 2 ints per bin) and then le[i_k] and le[min(i_k + 1, L)]: one LDS round trip
// of the values, issued as batches (all map reads, all value reads, then the arithmetic: the
// volatile loads keep program order).  i_k <= L by the map's clamp, so every read is inside wt.
// g[i]: the positive gain of the slot's bin.
template <int L>
__device__ __forceinline__ void warp_gains(const float (&le)[L / 64 + 1], const int* wmap, float* wt, int lane,
                                           float (&g)[L / 64 + 1]) {
    constexpr int E = L / 64;
#pragma unroll
    for (int i = 0; i < E; ++i) wt[lane + 64 * i] = le[i];
    wt[lane == 0 ? L : L + 1] = le[E];
    wave_lds_sync();
    i2v mp[E + 1];
    float a[E + 1], b[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) mp[i] = lds_ld2i(&wmap[2 * ((i == E) ? L : lane + 64 * i)]);
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        a[i] = lds_ld(&wt[mp[i].x]);
        b[i] = lds_ld(&wt[min(mp[i].x + 1, L)]);
    }
#pragma unroll
    for (int i = 0; i <= E; ++i) {
        const float lw = __builtin_fmaf(__int_as_float(mp[i].y), b[i] - a[i], a[i]);
        g[i] = exp_hw(lw - le[i]);
    }
}

}  // namespace pv
