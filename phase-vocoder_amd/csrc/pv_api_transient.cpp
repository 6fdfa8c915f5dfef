// pv_api_transient.cpp — the transient phase reset of libpv (pv_set_transient; DESIGN.md
// §3.11): the handle's buffers, the switch, the caller's flags, the stand-alone onset strength,
// and the launches do_resynthesis (pv_api_batch.cpp) makes while the feature is on.
#include <algorithm>

#include "pv_host.hpp"

namespace pvhost {

namespace {

// (a query the runtime refuses — the null stream while another stream captures — counts as
// capturing: nothing may be allocated then either)
bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return cs != hipStreamCaptureStatusNone;
}

// allocated and zeroed once, under the handle's lock
pv_status reserve(pv_handle* h) {
    std::lock_guard<std::mutex> lk(h->tr_mu);
    if (h->d_tr_flags) return PV_OK;
    const size_t C = (size_t)std::max(h->cfg.max_channels, 1), T = (size_t)std::max(h->cfg.max_frames, 1);
    const size_t R = (size_t)std::max(h->max_runs, 1);
    DevBuf<unsigned char> flags;
    DevBuf<float2> strength;
    DevBuf<float> theta;
    DevBuf<int> prr;
    if (flags.alloc_zero(C * T) != hipSuccess || strength.alloc_zero(C * T) != hipSuccess ||
        theta.alloc_zero(C * R * h->bins_pad) != hipSuccess || prr.alloc_zero(C * R) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PV_ERR_NOMEM, "pv_transient_reserve: flags, strengths, reset offsets");
    }
    // (synchronised: the caller's stream may be a non-blocking one, which the null stream's
    // memsets would not order before its first launch)
    if (hipDeviceSynchronize() != hipSuccess) return fail(PV_ERR_HIP, "pv_transient_reserve: zeroing the buffers");
    h->d_tr_strength = std::move(strength);
    h->d_tr_theta = std::move(theta);
    h->d_tr_prr = std::move(prr);
    h->d_tr_flags = std::move(flags);
    return PV_OK;
}

pv_status check_handle(const char* fn, const pv_handle* h) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    if (h->mode != PV_MODE_STANDARD)
        return fail(PV_ERR_ARG, std::string(fn) + ": REF_COMPAT handle (the transient phase reset is the STANDARD time stretch's)");
    if (h->effect != PV_TIME_SHIFT)
        return fail(PV_ERR_ARG, std::string(fn) + ": PV_PITCH_SHIFT handle (the transient phase reset is the STANDARD time stretch's)");
    return PV_OK;
}

pv_status check_rows(const char* fn, const pv_handle* h, int channels, int frames, long long ld) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (channels > 1 && ld < frames) return fail(PV_ERR_ARG, std::string(fn) + ": ld < frames");
    return PV_OK;
}

}  // namespace

pv_status transient_ready(pv_handle* h, const char* fn, hipStream_t s) {
    bool have;
    {
        std::lock_guard<std::mutex> lk(h->tr_mu);
        have = h->d_tr_flags.p != nullptr;
    }
    if (have) return PV_OK;
    // an allocation cannot be captured: under capture the buffers must exist already
    if (capturing(s))
        return fail(PV_ERR_ARG, std::string(fn) + " under stream capture: call pv_transient_reserve first");
    return reserve(h);
}

pv_status transient_flags(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames, hipStream_t s) {
    const long long ld = std::max(h->cfg.max_frames, 1);
    if (h->transient == PV_TRANSIENT_DETECT) {
        pv::OnsetParams o{};
        o.spec = reinterpret_cast<const float2*>(spec);
        o.ld_spec = ld_spec;
        o.spec_stride = h->spec_stride;
        o.frames = frames;
        o.F = h->F;
        o.nruns = nruns_of(h, frames);
        o.packed = h->packed;
        o.dst = h->d_tr_strength;
        o.ld_dst = ld;
        PV_LAUNCH(h, KON, s, pv::launch_onset(h->L_syn, C, o, s));
    }
    pv::PickParams k{};
    k.strength = (h->transient == PV_TRANSIENT_DETECT) ? h->d_tr_strength.p : nullptr;
    k.ld_strength = ld;
    k.thr = h->transient_thr;
    k.flags = h->d_tr_flags;
    k.ld_flags = ld;
    k.prev_reset_run = h->d_tr_prr;
    k.frames = frames;
    k.F = h->F;
    k.nruns = nruns_of(h, frames);
    PV_LAUNCH(h, KPK, s, pv::launch_pick(C, k, s));
    return PV_OK;
}

pv_status transient_offsets(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames,
                            const int* carry, pv::SynParams* p, hipStream_t s) {
    const long long ld = std::max(h->cfg.max_frames, 1);
    pv::ResetParams r{};
    r.spec = reinterpret_cast<const float2*>(spec);
    r.ld_spec = ld_spec;
    r.spec_stride = h->spec_stride;
    r.frames = frames;
    r.F = h->F;
    r.nruns = nruns_of(h, frames);
    r.bins_pad = h->bins_pad;
    r.packed = h->packed;
    r.carry = carry;
    r.ek = h->d_ek;
    r.jk_mod = h->d_jk_mod;
    r.rho = h->rho;
    r.p_mod = h->p_mod;
    r.q = h->q;
    r.q_pow2 = h->q_pow2;
    r.inv_q = h->inv_q;
    r.flags = h->d_tr_flags;
    r.ld_flags = ld;
    r.theta = h->d_tr_theta;
    PV_LAUNCH(h, KRST, s, pv::launch_reset(h->L_syn, C, r, s));
    pv::set_reset_args(p, pv::ResetArgs{h->d_tr_flags, ld, h->d_tr_theta, h->d_tr_prr});
    return PV_OK;
}

}  // namespace pvhost

using namespace pvhost;

extern "C" {

pv_status pv_transient_reserve(pv_handle* h) {
    pv_status st = check_handle("pv_transient_reserve", h);
    if (st != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    return transient_ready(h, "pv_transient_reserve", nullptr);
}

pv_status pv_set_transient(pv_handle* h, int mode, float thr) {
    pv_status st = check_handle("pv_set_transient", h);
    if (st != PV_OK) return st;
    if (mode != PV_TRANSIENT_OFF && mode != PV_TRANSIENT_FLAGS && mode != PV_TRANSIENT_DETECT)
        return fail(PV_ERR_ARG, "pv_set_transient: mode must be PV_TRANSIENT_OFF, _FLAGS or _DETECT");
    if (thr == 0.0f) thr = PV_TRANSIENT_DEFAULT_THRESHOLD;
    if (!(thr > 0.0f && thr < 1.0f)) return fail(PV_ERR_ARG, "pv_set_transient: thr must be in (0, 1), or 0 for the default");
    if (mode != PV_TRANSIENT_OFF && (h->formant || h->pitch_formant))
        return fail(PV_ERR_ARG, "pv_set_transient: not with formant preservation on (pv_set_formant, pv_pitch_set_formant)");
    h->transient = mode;
    h->transient_thr = thr;
    return PV_OK;
}

int pv_get_transient(const pv_handle* h) { return h ? h->transient : 0; }

pv_status pv_transient_set_flags(pv_handle* h, const unsigned char* flags, long long ld, int channels, int frames,
                                 void* stream) {
    pv_status st = check_handle("pv_transient_set_flags", h);
    if (st != PV_OK || (st = check_rows("pv_transient_set_flags", h, channels, frames, ld)) != PV_OK) return st;
    if (channels == 0) return PV_OK;
    if (frames > 0 && !flags) return fail(PV_ERR_ARG, "null flags");
    DeviceGuard g(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    if ((st = transient_ready(h, "pv_transient_set_flags", s)) != PV_OK) return st;
    // the rows of these channels: zero, the caller's flags, frame 0's flag zero again
    const size_t pitch = (size_t)std::max(h->cfg.max_frames, 1);
    PV_HIP(hipMemset2DAsync(h->d_tr_flags, pitch, 0, pitch, (size_t)channels, s));
    if (frames > 0) {
        PV_HIP(hipMemcpy2DAsync(h->d_tr_flags, pitch, flags, (size_t)std::max(ld, (long long)frames), (size_t)frames,
                                (size_t)channels, hipMemcpyDeviceToDevice, s));
        PV_HIP(hipMemset2DAsync(h->d_tr_flags, pitch, 0, 1, (size_t)channels, s));
    }
    return PV_OK;
}

pv_status pv_transient_get_flags(pv_handle* h, unsigned char* flags, long long ld, int channels, int frames,
                                 void* stream) {
    pv_status st = check_handle("pv_transient_get_flags", h);
    if (st != PV_OK || (st = check_rows("pv_transient_get_flags", h, channels, frames, ld)) != PV_OK) return st;
    if (channels == 0 || frames == 0) return PV_OK;
    if (!flags) return fail(PV_ERR_ARG, "null flags");
    DeviceGuard g(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    if ((st = transient_ready(h, "pv_transient_get_flags", s)) != PV_OK) return st;
    PV_HIP(hipMemcpy2DAsync(flags, (size_t)std::max(ld, (long long)frames), h->d_tr_flags,
                            (size_t)std::max(h->cfg.max_frames, 1), (size_t)frames, (size_t)channels,
                            hipMemcpyDeviceToDevice, s));
    return PV_OK;
}

pv_status pv_onset_strength(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels, int frames,
                            pv_float2* dst, long long ld_dst, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (h->mode != PV_MODE_STANDARD) return fail(PV_ERR_UNSUPPORTED, "pv_onset_strength: STANDARD handles only");
    if (channels == 0 || frames == 0) return PV_OK;
    if (!spec || !dst) return fail(PV_ERR_ARG, "null spec/dst");
    if (ld_spec < (long long)frames * h->spec_stride) return fail(PV_ERR_ARG, "ld_spec < frames * spec_stride");
    if (channels > 1 && ld_dst < frames) return fail(PV_ERR_ARG, "pv_onset_strength: ld_dst < frames");
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    hipStream_t s = (hipStream_t)stream;
    pv::OnsetParams o{};
    o.spec = reinterpret_cast<const float2*>(spec);
    o.ld_spec = ld_spec;
    o.spec_stride = h->spec_stride;
    o.frames = frames;
    o.F = h->F;
    o.nruns = nruns_of(h, frames);
    o.packed = h->packed;
    o.dst = reinterpret_cast<float2*>(dst);
    o.ld_dst = ld_dst;
    PV_LAUNCH(h, KON, s, pv::launch_onset(h->L_syn, channels, o, s));
    return PV_OK;
}

}  // extern "C"
