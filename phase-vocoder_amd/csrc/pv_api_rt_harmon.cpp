// pv_api_rt_harmon.cpp — the real-time harmoniser of libpv (pv_rt_harmonizer_*):
// V voices of the real-time pitch map (pv_api_rt.cpp, §3.16) per channel from one analysis, each
// with a pitch ratio and a gain per pushed frame, mixed by the second of its two launches.  The
// captured callback is pv_api_rt.cpp's.
#include <string>
#include <vector>

#include "pv_host.hpp"

using namespace pvhost;

pv_status pvhost::rt_harmon_zero(pv_rt* rt, hipStream_t s) {
    const size_t C = (size_t)rt->channels, CV = C * (size_t)rt->harm_voices, BP = rt->h->bins_pad, N = rt->h->N;
    PV_HIP(hipMemsetAsync(rt->d_hprev.p, 0, sizeof(float2) * C * BP, s));
    PV_HIP(hipMemsetAsync(rt->d_hphi.p, 0, sizeof(unsigned) * CV * BP, s));
    PV_HIP(hipMemsetAsync(rt->d_hola.p, 0, sizeof(float) * CV * N, s));
    PV_HIP(hipMemsetAsync(rt->d_hstate.p, 0, sizeof(pv::RtMapState) * CV, s));
    PV_HIP(hipMemsetAsync(rt->d_hgprev.p, 0, sizeof(pv::RtHGain) * CV, s));
    PV_HIP(hipMemsetAsync(rt->d_hring.p, 0, sizeof(pv::RtHStep) * CV * (size_t)rt->harm_plan.ring_cap, s));
    PV_HIP(hipMemsetAsync(rt->d_hrow.p, 0, sizeof(float) * CV * (size_t)rt->harm_plan.row_len, s));
    return PV_OK;
}

extern "C" {

int pv_rt_harmonizer_max_voices(int n_samps) { return rt_harmonizer_max_voices(n_samps); }

pv_status pv_rt_harmonizer_reserve(pv_rt* rt, int voices, int quality, int max_nframes, float ratio_min,
                                   float ratio_max) {
    const char* fn = "pv_rt_harmonizer_reserve";
    const std::string f(fn);
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    pv_handle* h = rt->h;
    pv_status st = check_std_stretch(fn, h);
    if (st != PV_OK) return st;
    if (h->hs != h->hop) return fail(PV_ERR_UNSUPPORTED, f + ": the handle's out_hop must equal its hop (scale 1)");
    if (h->hop < 16) return fail(PV_ERR_UNSUPPORTED, f + ": the hop must be at least 16");
    const int vmax = rt_harmonizer_max_voices(h->N);
    if (vmax == 0 || pv::rt_hmap_max_voices(h->L_syn) != vmax)
        return fail(PV_ERR_UNSUPPORTED, f + ": no kernel for this n_samps");
    if (voices < 1 || voices > vmax)
        return fail(PV_ERR_ARG, f + ": voices must be in [1, " + std::to_string(vmax) + "] at this n_samps");
    if ((st = check_quality(fn, quality)) != PV_OK) return st;
    if (max_nframes <= 0) return fail(PV_ERR_ARG, f + ": max_nframes must be > 0");
    if (rt->exec) return fail(PV_ERR_ARG, f + ": a callback is captured (call it before pv_rt_capture)");
    RtPitchmapPlan plan{};
    if (!rt_pitchmap_plan(h->hop, quality, ratio_min, ratio_max, max_nframes, &plan))
        return fail(PV_ERR_ARG, f + ": 1/4 <= ratio_min <= ratio_max <= 4 (no NaN), (G + max_nframes) * hop < 2^28");
    if (plan.G > 64)
        return fail(PV_ERR_ARG, f + ": the range needs G = " + std::to_string(plan.G) + " callbacks of latency, above 64");
    DeviceGuard dg(h->cfg.device);
    const size_t C = (size_t)rt->channels, CV = C * (size_t)voices, BP = h->bins_pad, N = h->N;
    std::vector<float> win;
    var_window_table(quality, pv::kVarWinN, pv::kVarWinLen, win);
    DevBuf<float2> prev, wtab;
    DevBuf<unsigned> phi;
    DevBuf<float> ola, row;
    DevBuf<pv::RtMapState> state;
    DevBuf<pv::RtHStep> ring;
    DevBuf<pv::RtHGain> gprev;
    // (the rows first: the largest, so a capacity that cannot be had fails before anything else is taken)
    if (row.alloc(CV * (size_t)plan.row_len) != hipSuccess || ring.alloc(CV * (size_t)plan.ring_cap) != hipSuccess ||
        ola.alloc(CV * N) != hipSuccess || phi.alloc(CV * BP) != hipSuccess || prev.alloc(C * BP) != hipSuccess ||
        state.alloc(CV) != hipSuccess || gprev.alloc(CV) != hipSuccess ||
        wtab.upload(reinterpret_cast<const float2*>(win.data()), win.size() / 2) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PV_ERR_NOMEM, f + ": stream state, scratch rows and window table");
    }
    // a repeated reserve replaces the voices, the preset, the range and the capacity; the harmoniser's stream restarts
    PV_HIP(hipDeviceSynchronize());  // pushes in flight read the old buffers
    rt->d_hprev = std::move(prev);
    rt->d_hphi = std::move(phi);
    rt->d_hola = std::move(ola);
    rt->d_hstate = std::move(state);
    rt->d_hring = std::move(ring);
    rt->d_hgprev = std::move(gprev);
    rt->d_hrow = std::move(row);
    rt->d_hwin = std::move(wtab);
    rt->harm_plan = plan;
    rt->harm_voices = voices;
    rt->harm_quality = quality;
    rt->harm_max = max_nframes;
    rt->harm_rmin = ratio_min;
    rt->harm_rmax = ratio_max;
    if ((st = rt_harmon_zero(rt, nullptr)) != PV_OK || hipDeviceSynchronize() != hipSuccess) {
        rt->harm_on = 0;
        rt->harm_voices = 0;
        rt->callback = rt->pmap_on ? pv_rt::kPitchmapPush : rt->pitch_on ? pv_rt::kPitchPush : pv_rt::kPush;
        return st != PV_OK ? st : fail(PV_ERR_HIP, f + ": zeroing the stream state");
    }
    rt->harm_on = 1;
    rt->callback = pv_rt::kHarmonPush;
    return PV_OK;
}

int pv_rt_harmonizer_voices(const pv_rt* rt) { return (rt && rt->harm_on) ? rt->harm_voices : 0; }

int pv_rt_harmonizer_latency(const pv_rt* rt) { return (rt && rt->harm_on) ? rt->harm_plan.latency : 0; }

pv_status pv_rt_harmonizer_push(pv_rt* rt, const float* in, long long ldi, int nframes, const float* ratio,
                                const float* gain, long long ld_ctl, float* mix, long long ldo, float* voices_out,
                                long long ld_voice, pv_float2* spec, long long ld_spec, void* stream) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (!rt->harm_on) return fail(PV_ERR_ARG, "pv_rt_harmonizer_push: call pv_rt_harmonizer_reserve first");
    if (nframes > rt->harm_max)
        return fail(PV_ERR_ARG, "pv_rt_harmonizer_push: nframes > max_nframes of pv_rt_harmonizer_reserve");
    if (nframes < 0) return fail(PV_ERR_ARG, "negative nframes");
    if (nframes == 0) return PV_OK;
    pv_handle* h = rt->h;
    const int V = rt->harm_voices;
    if (!in || !mix) return fail(PV_ERR_ARG, "null in/mix");
    if (rt->channels > 1 && (ldi < (long long)nframes * h->hop || ldo < (long long)nframes * h->hop))
        return fail(PV_ERR_ARG, "ldi/ldo smaller than one callback");
    if ((ratio || gain) && rt->channels * V > 1 && ld_ctl < nframes) return fail(PV_ERR_ARG, "ld_ctl < nframes");
    if (voices_out && rt->channels * V > 1 && ld_voice < (long long)nframes * h->hop)
        return fail(PV_ERR_ARG, "ld_voice smaller than one callback");
    if (spec && rt->channels > 1 && ld_spec < (long long)nframes * h->spec_stride)
        return fail(PV_ERR_ARG, "ld_spec < nframes * spec_stride");
    DeviceGuard g(h->cfg.device);
    const RtPitchmapPlan& plan = rt->harm_plan;
    pv::RtHMapParams p{};
    p.rt = rt_params(rt, in, ldi, nframes, nullptr, 0, spec, ld_spec);
    p.voices = V;
    p.ratio = ratio;
    p.gain = gain;
    p.ld_ctl = ld_ctl;
    p.ratio_min = rt->harm_rmin;
    p.ratio_max = rt->harm_rmax;
    p.prev = rt->d_hprev;
    p.phi = rt->d_hphi;
    p.ola = rt->d_hola;
    p.st = rt->d_hstate;
    p.ring = rt->d_hring;
    p.ring_cap = (int)plan.ring_cap;
    p.row = rt->d_hrow;
    p.ld_row = plan.row_len;
    p.K = plan.K;
    pv::RtHVarParams v{};
    v.row = rt->d_hrow;
    v.ld_row = plan.row_len;
    v.K = plan.K;
    v.mix = mix;
    v.ldo = ldo;
    v.voices_out = voices_out;
    v.ld_voice = ld_voice;
    v.st = rt->d_hstate;
    v.ring = rt->d_hring;
    v.ring_cap = (int)plan.ring_cap;
    v.gprev = rt->d_hgprev;
    v.win = rt->d_hwin;
    v.win_scale = (float)((double)pv::kVarWinN / resample_zero_crossings(rt->harm_quality) * 0x1p-32);
    v.channels = rt->channels;
    v.voices = V;
    v.nframes = nframes;
    v.hop = h->hop;
    v.G = plan.G;
    v.rolloff = resample_rolloff(rt->harm_quality);
    v.Z = resample_zero_crossings(rt->harm_quality);
    hipStream_t s = (hipStream_t)stream;
    prof_tick(h);
    PV_LAUNCH(h, KRTH, s, pv::launch_rt_hmap(h->L_syn, rt->phase_lock, p, s));
    PV_LAUNCH(h, KRTHR, s, pv::launch_rt_hresample(v, s));
    return PV_OK;
}

pv_status pv_rt_harmonizer_host_controls(pv_rt* rt, float** host_ratio, float** host_gain) {
    if (!rt || !rt->exec) return fail(PV_ERR_ARG, "no captured callback (pv_rt_capture)");
    if (rt->g_kind != pv_rt::kHarmonPush)
        return fail(PV_ERR_ARG, "pv_rt_harmonizer_host_controls: the captured callback is not pv_rt_harmonizer_push");
    if (host_ratio) *host_ratio = rt->h_ratio;
    if (host_gain) *host_gain = rt->h_gain;
    return PV_OK;
}

}  // extern "C"
