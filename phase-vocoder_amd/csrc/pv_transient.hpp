// pv_transient.hpp — transient phase reset of the STANDARD time stretch (pv_set_transient;
// DESIGN.md §3.11): the per-wave reset state of k_synthesis in the reset modes (pv_syn_kernel.hpp,
// instantiated in pv_transient.hip) and the reset offset both that kernel and k_reset compute.
//
// At a flagged frame t0 every bin is put down with its analysis phase; from then on the closed
// form of §3.3 carries one more additive offset per bin,
//   Theta[k] = fract(-(closed(t0)[k] / 2 pi - phi(t0)[k] / 2 pi))   (revolutions, in [0, 1)),
// constant until the next flagged frame.  closed / 2 pi - phi / 2 pi is what the locked
// propagation computes (synth_frame's phc with rho / 2 pi - 1 / 2 pi in place of rho / 2 pi), so
// one definition serves the unlocked and the locked synthesis.  Theta is a tolerance quantity;
// the unwrap counts, the run records and the carries are the plain modes'.
#pragma once
#include "pv_device.hpp"
#include "pv_lock.hpp"

namespace pv {

constexpr bool mode_is_reset(int mode) { return mode == kModeReset || mode == kModeLockedReset; }

// Theta from the locked form of the output phase (revolutions)
__device__ __forceinline__ float reset_offset(float locked_rev) { return __builtin_amdgcn_fractf(-locked_rev); }

// synth_frame's reset argument: off, or the wave's Theta registers (bin k = lane + 64 i in slot
// i, bin L in slot E of lane 0) and the frame's flag (wave-uniform)
struct NoReset {
    static constexpr bool ON = false;
};
template <int E>
struct ResetRef {
    static constexpr bool ON = true;
    float (&th)[E + 1];
    bool flag;
};

// syn_run's reset argument: off, or the Theta registers (initialised by the caller from the
// last flagged run before this one, or 0) and the flag bytes of the run's frames
struct NoResetRun {
    static constexpr bool ON = false;
};
template <int E>
struct ResetRun {
    static constexpr bool ON = true;
    float (&th)[E + 1];
    const unsigned char* flags;  // flags[u], u < nfr: frame t0 + u is flagged
};

}  // namespace pv
