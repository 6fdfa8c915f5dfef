// pv_resident.hpp — the two frame bodies of the channel-resident STANDARD time stretch
// (k_resident, pv_resident.hip): one analysis frame whose {mag, phase} row goes to LDS, and the
// LDS carve-up the roles share.  The analysis frame calls the pieces k_std_analysis is made of
// (pv_frame.hpp: fft_run, bin_l_real, polar_pair), so a row holds the bits that kernel writes to
// the spectrum; the synthesis side calls synth_frame, ola_add and ola_shift itself.
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

// The waves of a workgroup meet here.  Only LDS traffic has to be complete: the rows travel
// through LDS alone, so a wave's global loads and stores stay in flight across the barrier.
__device__ __forceinline__ void res_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One analysis frame from its windowed samples z: the row of bins 0 .. L in natural order.
template <int L>
__device__ __forceinline__ void res_ana_frame(float2 (&z)[Geo<L>::E], float2* tile, const float2* twl,
                                              const float2* twsl, const float2 (&tw0)[Geo<L>::E], int lane,
                                              float2* row) {
    constexpr int E = Geo<L>::E;
    fft_run<L, false, false>(z, tile, twl, tw0, lane);
    float magL, phL;
    bin_l_real<L, true>(z, twsl, magL, phL);
    static_for<0, E / 2>([&](auto ic) {
        constexpr int i0 = 2 * decltype(ic)::value;
        polar_pair<L, i0>(z, twsl, lane, [&](auto cc, float mag, float ph) {
            row[lane + 64 * (i0 + decltype(cc)::value)] = make_float2(mag, ph);
        });
    });
    if (lane == 0) row[L] = make_float2(magL, phL);
    wave_lds_sync();
}

}  // namespace pv
