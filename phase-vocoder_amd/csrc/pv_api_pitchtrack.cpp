// pv_api_pitchtrack.cpp — the pitch tracker and the correction curve of libpv (pv_pitch_track,
// pv_pitch_correct_plan): the checks and the one launch of the first, the
// C entry of the second (the recipe is pvtab::pitch_correct_plan, pure host).
#include <cmath>

#include "pv_host.hpp"

using namespace pvhost;

extern "C" {

pv_status pv_pitch_track(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels, int frames,
                         int tau_min, int tau_max, float kappa, pv_float2* dst, long long ld_dst, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (h->mode != PV_MODE_STANDARD) return fail(PV_ERR_UNSUPPORTED, "pv_pitch_track: STANDARD handles only");
    if (tau_min < 2 || tau_max < tau_min || tau_max > h->N / 2 - 1)
        return fail(PV_ERR_ARG, "pv_pitch_track: the lags must satisfy 2 <= tau_min <= tau_max <= N/2 - 1");
    if (!(kappa >= 0.0f && kappa <= 1.0f))
        return fail(PV_ERR_ARG, "pv_pitch_track: kappa must be in (0, 1], or 0 for the default");
    if (kappa == 0.0f) kappa = PV_PITCH_TRACK_DEFAULT_KAPPA;
    if (channels == 0 || frames == 0) return PV_OK;
    if (!spec || !dst) return fail(PV_ERR_ARG, "null spec/dst");
    if ((st = check_ld_spec(h, frames, ld_spec)) != PV_OK) return st;
    if (channels > 1 && ld_dst < frames) return fail(PV_ERR_ARG, "pv_pitch_track: ld_dst < frames");
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    hipStream_t s = (hipStream_t)stream;
    pv::PitchParams p{};
    p.spec = reinterpret_cast<const float2*>(spec);
    p.ld_spec = ld_spec;
    p.spec_stride = h->spec_stride;
    p.frames = frames;
    p.F = h->F;
    p.nruns = nruns_of(h, frames);
    p.packed = h->packed;
    p.tau_min = tau_min;
    p.tau_max = tau_max;
    p.kappa = kappa;
    p.tw = syn_v3_table(h);
    p.tws = h->d_tws_syn;
    p.dst = reinterpret_cast<float2*>(dst);
    p.ld_dst = ld_dst;
    PV_LAUNCH(h, KPT, s, pv::launch_pitch(h->L_syn, channels, p, s));
    return PV_OK;
}

pv_status pv_pitch_correct_plan(const pv_float2* track, int frames, const double* pos, int n,
                                const pv_pitch_correct* cfg, double* ratio) {
    if (!track || !cfg || !ratio) return fail(PV_ERR_ARG, "pv_pitch_correct_plan: null argument");
    if (cfg->abi_version != PV_ABI_VERSION)
        return fail(PV_ERR_ARG, "pv_pitch_correct.abi_version != PV_ABI_VERSION (caller built against another pv.h)");
    if (!pitch_correct_plan(track, frames, pos, n, *cfg, ratio))
        return fail(PV_ERR_ARG, "pv_pitch_correct_plan: frames >= 1, n >= 1, a4 > 0 and finite, scale_mask in [1, 4095], "
                                "strength_min not NaN, retune in (0, 1], every position finite");
    return PV_OK;
}

}  // extern "C"
