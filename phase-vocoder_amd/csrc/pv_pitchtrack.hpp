// pv_pitchtrack.hpp — the pitch tracker (pv_pitch_track): the parameter block
// and the launch of k_pitch (pv_pitchtrack.hip).  Plain declarations: included by the kernel's
// translation unit and by the host (pv_api_pitchtrack.cpp).
#pragma once
#include <hip/hip_runtime.h>

namespace pv {

// {f0, strength} of every frame from the analysis rows' magnitudes: the window-corrected
// circular autocorrelation of the frame (the inverse real FFT of mag^2), McLeod and Wyvill's
// key maximum over the lags tau_min .. tau_max, a parabola through the pick's neighbours
struct PitchParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, frames, F, nruns;
    int packed;                        // PV_SPEC_PACKED rows
    int tau_min, tau_max;              // 2 <= tau_min <= tau_max <= N/2 - 1
    float kappa;                       // (0, 1]
    const float2* tw;                  // the v3 pass table of the L-point FFT
    const float2* tws;                 // e^{-2 pi i k/N}, k <= L
    float2* dst;                       // dst[c * ld_dst + t] = {f0 (cycles per sample), strength}
    long long ld_dst;
};

// L = N/2 in {128, 256, 512, 1024}; hipErrorInvalidValue otherwise
hipError_t launch_pitch(int L, int channels, const PitchParams& p, hipStream_t s);

}  // namespace pv
