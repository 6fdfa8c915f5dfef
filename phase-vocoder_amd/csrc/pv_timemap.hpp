// pv_timemap.hpp — the time-map stretch (pv_timemap_process): a phase as a
// 32-bit fraction of a turn and the per-wave map state of k_synthesis in the map modes
// (pv_syn_kernel.hpp, instantiated in pv_timemap.hip).
//
// Output frame u is built at the fractional analysis position i_u + a_u: its magnitude is the
// fp32 lerp of rows i_u and i_u + 1, its phase Phi(u) the sum of the measured phase steps
// Delta(i) = P(i + 1) - P(i) of the frames before it.  The synthesis hop is the analysis hop, so
// the unwrap integers drop out and the sum is an integer scan modulo 2^32: exact and associative,
// whatever the run length.
#pragma once
#include "pv_device.hpp"
#include "pv_kernels.h"
#include "pv_lock.hpp"

namespace pv {

constexpr bool mode_is_map(int mode) { return mode == kModeMap || mode == kModeLockedMap; }

// P: the analysis phase phi (radians, |phi| <= pi (1 + eps), finite: contract v4) as a fraction of
// a turn in units of 2^-32.  t = phi / 2 pi is the synthesis' own multiply; t 2^31 is exact and
// at most 2^30 (1 + eps) in magnitude, so the conversion never saturates; ties to even.
__device__ __forceinline__ unsigned phase_turns(float phi) {
    const float t = phi * kInv2Pi;
    return ((unsigned)(int)__builtin_rintf(t * 0x1p31f)) << 1;
}
// ... and back, for sin / cos: revolutions in [-1/2, 1/2]
__device__ __forceinline__ float turns_rev(unsigned psi) { return (float)(int)psi * 0x1p-32f; }

// syn_run's map argument: off, or the run's map entries and the number of analysed rows (row
// `aframes`, one past the end, reads as magnitude 0 and phase step 0 and is never loaded; the
// host has checked i_u <= aframes - 1 for every entry)
struct NoMapRun {
    static constexpr bool ON = false;
};
struct MapRun {
    static constexpr bool ON = true;
    const MapEntry* map;  // map[u], u < nfr: output frame t0 + u
    int aframes;
};

}  // namespace pv
