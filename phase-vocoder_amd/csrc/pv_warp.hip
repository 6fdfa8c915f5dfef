// pv_warp.hip — K3 of the STANDARD time stretch with the envelope warp (pv_pitch_set_formant;
// DESIGN.md §3.10), formant preservation for the stretch-and-resample pitch shift: the
// instantiations of k_synthesis (pv_syn_kernel.hpp) in the warp and the locked warp mode and
// their launch.  The frames scale every magnitude by exp(lw - le): the frame's log envelope
// (k_envelope's row, loaded one frame ahead as in the formant mode) read at the bin's warp
// position (synth_frame's kModeWarp / kModeLockedWarp, warp_gains in pv_warp.hpp).  Locked: the
// output phases are the locked stretch's (lock_offsets), with every peak and owner decision
// made on the unscaled magnitudes.  No self-tracked-prefetch variants.
//
// A translation unit of its own: the kernels compile next to the other modes', and their
// registers are checked file by file (tests/test_pitch_formant_ref.py).
#include "pv_syn_kernel.hpp"

namespace pv {

// the kernel of launch_synthesis_locked for the same geometry (launch_syn_plain), up to
// L = 1024; the warp map travels in the pitch map's fields
hipError_t launch_synthesis_warp(int L, int lock, int channels, const SynParams& p, hipStream_t s) {
    if (!p.env || !p.src_first || !p.src_cnt) return hipErrorInvalidValue;
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    const int dt = qp ? syn_dt(L, p.hs) : 0;
    if (lock) return qp ? launch_syn_plain<kModeLockedWarp, true, 1024>(L, dt, grid, p, s)
                        : launch_syn_plain<kModeLockedWarp, false, 1024>(L, dt, grid, p, s);
    return qp ? launch_syn_plain<kModeWarp, true, 1024>(L, dt, grid, p, s)
              : launch_syn_plain<kModeWarp, false, 1024>(L, dt, grid, p, s);
}

}  // namespace pv
