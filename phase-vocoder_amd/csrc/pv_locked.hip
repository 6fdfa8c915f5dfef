// pv_locked.hip — K3 of the STANDARD time stretch with identity phase locking
// (pv_set_phase_lock): the instantiations of k_synthesis (pv_syn_kernel.hpp)
// in the locked mode and their launch.  The frames take every bin's output phase from the
// magnitude peak that owns the bin (synth_frame's kModeLocked, lock_offsets in pv_lock.hpp).
//
// A translation unit of its own: the kernels compile next to the other modes', and their
// registers are checked file by file (tests/test_phase_lock_ref.py).
#include "pv_syn_kernel.hpp"

namespace pv {

// the kernel of launch_synthesis's mode 0 for the same geometry (launch_syn_plain), up to
// L = 2048
hipError_t launch_synthesis_locked(int L, int channels, const SynParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    const int dt = qp ? syn_dt(L, p.hs) : 0;
    return qp ? launch_syn_plain<kModeLocked, true, 2048>(L, dt, grid, p, s)
              : launch_syn_plain<kModeLocked, false, 2048>(L, dt, grid, p, s);
}

}  // namespace pv
