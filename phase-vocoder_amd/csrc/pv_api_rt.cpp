// pv_api_rt.cpp — real-time mode of libpv: pv_rt (pv_host.hpp) is a pv_handle (tables) +
// per-channel stream state + an optional captured graph of one callback (pinned host in ->
// device -> pv_rt_push -> pinned host out); the real-time pitch shift adds the locked stretch
// and the streaming resampler, the real-time pitch map a pitch ratio per pushed
// frame (pv_rt_pitchmap_*); the real-time harmoniser (pv_api_rt_harmon.cpp;
// DESIGN.md §3.17) shares the captured callback.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pv_host.hpp"

using namespace pvhost;

pv::RtParams pvhost::rt_params(const pv_rt* rt, const float* in, long long ldi, int nframes, float* out, long long ldo,
                       pv_float2* spec, long long ld_spec) {
    const pv_handle* h = rt->h;
    pv::RtParams p{};
    p.in = in;
    p.ldi = ldi;
    p.out = out;
    p.ldo = ldo;
    p.spec = reinterpret_cast<float2*>(spec);
    p.ld_spec = ld_spec;
    p.spec_stride = h->spec_stride;
    p.channels = rt->channels;
    p.nframes = nframes;
    p.hop = h->hop;
    p.hs = h->hs;
    p.bins_pad = h->bins_pad;
    p.hist = rt->d_hist;
    p.ola = rt->d_ola;
    p.phprev = rt->d_phprev;
    p.M = rt->d_M;
    p.tcount = rt->d_tcount;
    p.win = h->d_win;
    p.gain = h->d_gain;
    p.tw = h->d_tw_syn;
    p.tws = h->d_tws_syn;
    p.ek = h->d_ek;
    p.jk_mod = h->d_jk_mod;
    p.src_first = h->d_src_first;
    p.src_cnt = h->d_src_cnt;
    p.rho = h->rho;
    p.p_mod = h->p_mod;
    p.q = h->q;
    p.q_pow2 = h->q_pow2;
    p.inv_q = h->inv_q;
    return p;
}
namespace {
// the captured callback; the stream stays for the next capture
void rt_release_graph(pv_rt* rt) {
    if (rt->exec) (void)hipGraphExecDestroy(rt->exec);
    if (rt->graph) (void)hipGraphDestroy(rt->graph);
    rt->exec = nullptr;
    rt->graph = nullptr;
    rt->h_in.reset();
    rt->h_out.reset();
    rt->d_in.reset();
    rt->d_out.reset();
    rt->h_ratio.reset();
    rt->d_ratio.reset();
    rt->m_ratio = nullptr;
    rt->h_gain.reset();
    rt->d_gain.reset();
    rt->m_gain = nullptr;
    rt->g_nframes = 0;
    rt->g_kind = pv_rt::kPush;
}
// samples per frame a callback emits: hop once pv_rt_pitch_reserve, pv_rt_pitchmap_reserve or
// pv_rt_harmonizer_reserve has succeeded, else out hop
int rt_out_hop(const pv_rt* rt) { return rt->callback != pv_rt::kPush ? rt->h->hop : rt->h->hs; }
// what a callback runs: the push of the later successful reserve, else pv_rt_push (ratio: the
// pitch map's [channels][nframes] ratios, or the harmoniser's [channels][voices][nframes] beside
// its gains; the harmoniser's callback emits the mix)
pv_status rt_callback_push(pv_rt* rt, const float* in, long long ldi, int nframes, const float* ratio,
                           const float* gain, float* out, long long ldo, hipStream_t s) {
    switch (rt->callback) {
        case pv_rt::kHarmonPush:
            return pv_rt_harmonizer_push(rt, in, ldi, nframes, ratio, gain, nframes, out, ldo, nullptr, 0, nullptr, 0, s);
        case pv_rt::kPitchmapPush:
            return pv_rt_pitchmap_push(rt, in, ldi, nframes, ratio, nframes, out, ldo, nullptr, 0, s);
        case pv_rt::kPitchPush: return pv_rt_pitch_push(rt, in, ldi, nframes, out, ldo, nullptr, 0, s);
        default: return pv_rt_push(rt, in, ldi, nframes, out, ldo, nullptr, 0, s);
    }
}
// the real-time pitch map's stream state, zeroed (a stream's start)
pv_status rt_pitchmap_zero(pv_rt* rt, hipStream_t s) {
    const size_t C = (size_t)rt->channels, BP = rt->h->bins_pad;
    PV_HIP(hipMemsetAsync(rt->d_mprev.p, 0, sizeof(float2) * C * BP, s));
    PV_HIP(hipMemsetAsync(rt->d_mphi.p, 0, sizeof(unsigned) * C * BP, s));
    PV_HIP(hipMemsetAsync(rt->d_mstate.p, 0, sizeof(pv::RtMapState) * C, s));
    PV_HIP(hipMemsetAsync(rt->d_mring.p, 0, sizeof(long long) * C * (size_t)rt->pmap_plan.ring_cap, s));
    PV_HIP(hipMemsetAsync(rt->d_mrow.p, 0, sizeof(float) * C * (size_t)rt->pmap_plan.row_len, s));
    return PV_OK;
}
struct RtDeleter {
    void operator()(pv_rt* rt) const { pv_rt_destroy(rt); }
};
// no event records inside a captured graph: the profiler is off for the guard's life
struct ProfOff {
    pv_handle* h;
    bool was;
    explicit ProfOff(pv_handle* hh) : h(hh), was(hh->prof.enabled) { h->prof.enabled = false; }
    ~ProfOff() { h->prof.enabled = was; }
};
}  // namespace

extern "C" {

void pv_rt_destroy(pv_rt* rt) {
    if (!rt) return;
    pv_handle* h = rt->h;
    DeviceGuard g(h->cfg.device);
    rt_release_graph(rt);
    if (rt->g_stream) (void)hipStreamDestroy(rt->g_stream);
    delete rt;  // frees its stream state, before the handle's tables
    pv_destroy(h);
}

pv_status pv_rt_reset(pv_rt* rt, void* stream) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    DeviceGuard g(rt->h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    const size_t C = (size_t)rt->channels, N = rt->h->N, BP = rt->h->bins_pad;
    PV_HIP(hipMemsetAsync(rt->d_hist.p, 0, sizeof(float) * C * N, s));
    PV_HIP(hipMemsetAsync(rt->d_ola.p, 0, sizeof(float) * C * N, s));
    PV_HIP(hipMemsetAsync(rt->d_phprev.p, 0, sizeof(float) * C * BP, s));
    PV_HIP(hipMemsetAsync(rt->d_M.p, 0, sizeof(int) * C * BP, s));
    PV_HIP(hipMemsetAsync(rt->d_tcount.p, 0, sizeof(unsigned) * C, s));
    if (rt->d_prow) PV_HIP(hipMemsetAsync(rt->d_prow.p, 0, sizeof(float) * C * (size_t)rt->ld_prow, s));
    if (rt->pmap_on) {
        pv_status st = rt_pitchmap_zero(rt, s);
        if (st != PV_OK) return st;
    }
    if (rt->harm_on) return rt_harmon_zero(rt, s);
    return PV_OK;
}

pv_status pv_rt_create(const pv_config* cfg, int channels, pv_rt** out) {
    if (!cfg || !out) return fail(PV_ERR_ARG, "null argument");
    // the version first: no other field of a caller's struct is read before it matches
    pv_status st = check_abi(cfg);
    if (st != PV_OK) return st;
    if (cfg->tables_external) return fail(PV_ERR_UNSUPPORTED, "tables_external: batch handles only");
    *out = nullptr;
    if (cfg->mode != PV_MODE_STANDARD)
        return fail(PV_ERR_UNSUPPORTED, "real-time mode runs the STANDARD pipeline only");
    if (cfg->spec_layout != PV_SPEC_NATURAL)
        return fail(PV_ERR_UNSUPPORTED, "real-time mode: natural spectrum rows only");
    if (channels <= 0) return fail(PV_ERR_ARG, "channels must be > 0");
    pv_config c = *cfg;
    c.max_channels = channels;
    c.max_frames = std::max(c.max_frames, 1);
    pv_handle* h = nullptr;
    if ((st = pv_create(&c, &h)) != PV_OK) return st;
    std::unique_ptr<pv_rt, RtDeleter> rt(new pv_rt());  // owns the handle from here on
    rt->h = h;
    rt->channels = channels;
    if (pv::rt_lds_bytes(h->L_syn) == 0) return fail(PV_ERR_UNSUPPORTED, "real-time mode: n_samps in [256, 2048]");
    DeviceGuard g(cfg->device);
    const size_t C = (size_t)channels, N = h->N, BP = h->bins_pad;
    auto alloc = [&](auto& buf, size_t n) -> pv_status {
        hipError_t e = buf.alloc(n);
        if (e != hipSuccess) return fail(PV_ERR_NOMEM, std::string("pv_rt_create: ") + hipGetErrorString(e));
        return PV_OK;
    };
    if ((st = alloc(rt->d_hist, C * N)) != PV_OK || (st = alloc(rt->d_ola, C * N)) != PV_OK ||
        (st = alloc(rt->d_phprev, C * BP)) != PV_OK || (st = alloc(rt->d_M, C * BP)) != PV_OK ||
        (st = alloc(rt->d_tcount, C)) != PV_OK)
        return st;
    if ((st = pv_rt_reset(rt.get(), nullptr)) != PV_OK) return st;
    if (hipDeviceSynchronize() != hipSuccess) return fail(PV_ERR_HIP, "pv_rt_create: reset failed");
    *out = rt.release();
    return PV_OK;
}

pv_status pv_rt_push(pv_rt* rt, const float* in, long long ldi, int nframes, float* out,
                     long long ldo, pv_float2* spec, long long ld_spec, void* stream) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (nframes < 0) return fail(PV_ERR_ARG, "negative nframes");
    if (nframes == 0) return PV_OK;
    pv_handle* h = rt->h;
    if (!in || !out) return fail(PV_ERR_ARG, "null in/out");
    if (rt->channels > 1 && (ldi < (long long)nframes * h->hop || ldo < (long long)nframes * h->hs))
        return fail(PV_ERR_ARG, "ldi/ldo smaller than one callback");
    if (spec && rt->channels > 1 && ld_spec < (long long)nframes * h->spec_stride)
        return fail(PV_ERR_ARG, "ld_spec < nframes * spec_stride");
    DeviceGuard g(h->cfg.device);
    const pv::RtParams p = rt_params(rt, in, ldi, nframes, out, ldo, spec, ld_spec);
    hipStream_t s = (hipStream_t)stream;
    prof_tick(h);  // one public call: the profile stride counts pv_rt_push calls too
    PV_LAUNCH(h, KRT, s, pv::launch_rt(h->L_syn, h->pitch ? 2 : rt->phase_lock ? pv::kRtModeLocked : 0, p, s));
    return PV_OK;
}

// ---- real-time pitch shift: the locked stretch and the streaming resampler
pv_status pv_rt_set_phase_lock(pv_rt* rt, int lock) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (lock != 0 && lock != 1) return fail(PV_ERR_ARG, "pv_rt_set_phase_lock: lock must be 0 or 1");
    pv_status st = check_std_stretch("pv_rt_set_phase_lock", rt->h);
    if (st != PV_OK) return st;
    if (rt->exec) return fail(PV_ERR_ARG, "pv_rt_set_phase_lock: a callback is captured (call it before pv_rt_capture)");
    rt->phase_lock = lock;
    return PV_OK;
}

int pv_rt_get_phase_lock(const pv_rt* rt) { return rt ? rt->phase_lock : 0; }

pv_status pv_rt_pitch_reserve(pv_rt* rt, int quality, int max_nframes) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    pv_handle* h = rt->h;
    pv_status st = check_std_stretch("pv_rt_pitch_reserve", h);
    if (st != PV_OK || (st = check_quality("pv_rt_pitch_reserve", quality)) != PV_OK) return st;
    if (max_nframes <= 0) return fail(PV_ERR_ARG, "pv_rt_pitch_reserve: max_nframes must be > 0");
    if (rt->exec) return fail(PV_ERR_ARG, "pv_rt_pitch_reserve: a callback is captured (call it before pv_rt_capture)");
    const long long g = gcd_ll(h->hs, h->hop);
    const long long P = h->hs / g, Q = h->hop / g;
    if (P > 4 * Q || Q > 4 * P) return fail(PV_ERR_UNSUPPORTED, "pv_rt_pitch_reserve: out_hop / hop in [1/4, 4]");
    const int W = (P == Q) ? 0 : resample_half_width((int)P, (int)Q, quality);
    const int H = (2 * W + 3) & ~3;
    const long long D = (P == Q) ? 0 : (long long)W * Q / P;
    // the kernel's dividend (u P + W Q - D P, u < max_nframes * hop) in 32 bits
    if ((long long)max_nframes * h->hop * P + (long long)W * Q > 0x7fffffffLL)
        return fail(PV_ERR_ARG, "pv_rt_pitch_reserve: max_nframes too large");
    DeviceGuard dg(h->cfg.device);
    DevBuf<float> row, tab;
    long long ld = 0;
    if (P != Q) {
        std::vector<float> t((size_t)Q * 2 * W);
        for (int r = 0; r < (int)Q; ++r) resample_row((int)P, (int)Q, quality, W, r, t.data() + (size_t)r * 2 * W);
        ld = ((long long)H + (long long)max_nframes * h->hs + 3) & ~3LL;
        const size_t row_n = (size_t)ld * (size_t)rt->channels;
        if (row.alloc(row_n) != hipSuccess || tab.alloc(t.size()) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PV_ERR_NOMEM, "pv_rt_pitch_reserve: scratch rows / coefficient table");
        }
        if (hipMemset(row.p, 0, sizeof(float) * row_n) != hipSuccess ||
            hipMemcpy(tab.p, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess)
            return fail(PV_ERR_HIP, "pv_rt_pitch_reserve: uploading the coefficient table");
    }
    // a repeated reserve replaces the quality and the capacity; the resampler's history restarts
    if (rt->d_prow || rt->d_ptab) (void)hipDeviceSynchronize();  // pushes in flight read the old rows and table
    rt->d_prow = std::move(row);
    rt->d_ptab = std::move(tab);
    rt->ld_prow = ld;
    rt->pitch_P = (int)P;
    rt->pitch_Q = (int)Q;
    rt->pitch_W = W;
    rt->pitch_H = H;
    rt->pitch_D = (int)D;
    rt->pitch_max = max_nframes;
    rt->pitch_on = 1;
    rt->callback = pv_rt::kPitchPush;
    return PV_OK;
}

int pv_rt_pitch_latency(const pv_rt* rt) { return (rt && rt->pitch_on) ? rt->pitch_D : 0; }

pv_status pv_rt_pitch_push(pv_rt* rt, const float* in, long long ldi, int nframes, float* out, long long ldo,
                           pv_float2* spec, long long ld_spec, void* stream) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (!rt->pitch_on) return fail(PV_ERR_ARG, "pv_rt_pitch_push: call pv_rt_pitch_reserve first");
    if (nframes > rt->pitch_max) return fail(PV_ERR_ARG, "pv_rt_pitch_push: nframes > max_nframes of pv_rt_pitch_reserve");
    // out hop = hop: no resampling, the stretch writes `out`
    if (!rt->d_ptab) return pv_rt_push(rt, in, ldi, nframes, out, ldo, spec, ld_spec, stream);
    if (nframes < 0) return fail(PV_ERR_ARG, "negative nframes");
    if (nframes == 0) return PV_OK;
    pv_handle* h = rt->h;
    if (!in || !out) return fail(PV_ERR_ARG, "null in/out");
    if (rt->channels > 1 && ldo < (long long)nframes * h->hop) return fail(PV_ERR_ARG, "ldo smaller than one callback");
    pv_status st = pv_rt_push(rt, in, ldi, nframes, rt->d_prow + rt->pitch_H, rt->ld_prow, spec, ld_spec, stream);
    if (st != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    pv::RtResampleParams p{};
    p.row = rt->d_prow;
    p.ld_row = rt->ld_prow;
    p.out = out;
    p.ldo = ldo;
    p.tab = rt->d_ptab;
    p.channels = rt->channels;
    p.n_new = nframes * h->hs;
    p.n_out = nframes * h->hop;
    p.P = rt->pitch_P;
    p.Q = rt->pitch_Q;
    p.W = rt->pitch_W;
    p.H = rt->pitch_H;
    p.off = (unsigned)((long long)rt->pitch_W * rt->pitch_Q - (long long)rt->pitch_D * rt->pitch_P);
    hipStream_t s = (hipStream_t)stream;
    PV_LAUNCH(h, KRTR, s, pv::launch_rt_resample(p, s));
    return PV_OK;
}

// ---- real-time pitch map: a pitch ratio per pushed frame
pv_status pv_rt_pitchmap_reserve(pv_rt* rt, int quality, int max_nframes, float ratio_min, float ratio_max) {
    const char* fn = "pv_rt_pitchmap_reserve";
    const std::string f(fn);
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    pv_handle* h = rt->h;
    pv_status st = check_std_stretch(fn, h);
    if (st != PV_OK) return st;
    if (h->hs != h->hop) return fail(PV_ERR_UNSUPPORTED, f + ": the handle's out_hop must equal its hop (scale 1)");
    if (h->hop < 16) return fail(PV_ERR_UNSUPPORTED, f + ": the hop must be at least 16");
    if (!pv::rt_map_kernel(h->L_syn)) return fail(PV_ERR_UNSUPPORTED, f + ": no kernel for this n_samps");
    if ((st = check_quality(fn, quality)) != PV_OK) return st;
    if (max_nframes <= 0) return fail(PV_ERR_ARG, f + ": max_nframes must be > 0");
    if (rt->exec) return fail(PV_ERR_ARG, f + ": a callback is captured (call it before pv_rt_capture)");
    RtPitchmapPlan plan{};
    if (!rt_pitchmap_plan(h->hop, quality, ratio_min, ratio_max, max_nframes, &plan))
        return fail(PV_ERR_ARG, f + ": 1/4 <= ratio_min <= ratio_max <= 4 (no NaN), (G + max_nframes) * hop < 2^28");
    if (plan.G > 64)
        return fail(PV_ERR_ARG, f + ": the range needs G = " + std::to_string(plan.G) + " callbacks of latency, above 64");
    DeviceGuard dg(h->cfg.device);
    const size_t C = (size_t)rt->channels, BP = h->bins_pad;
    std::vector<float> win;
    var_window_table(quality, pv::kVarWinN, pv::kVarWinLen, win);
    DevBuf<float2> prev, wtab;
    DevBuf<unsigned> phi;
    DevBuf<pv::RtMapState> state;
    DevBuf<long long> ring;
    DevBuf<float> row;
    // (the rows first: the largest, so a capacity that cannot be had fails before anything else is taken)
    if (row.alloc(C * (size_t)plan.row_len) != hipSuccess || ring.alloc(C * (size_t)plan.ring_cap) != hipSuccess ||
        prev.alloc(C * BP) != hipSuccess || phi.alloc(C * BP) != hipSuccess || state.alloc(C) != hipSuccess ||
        wtab.upload(reinterpret_cast<const float2*>(win.data()), win.size() / 2) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PV_ERR_NOMEM, f + ": stream state, scratch rows and window table");
    }
    // a repeated reserve replaces the preset, the range and the capacity; the pitch map's stream restarts
    PV_HIP(hipDeviceSynchronize());  // pushes in flight read the old buffers
    rt->d_mprev = std::move(prev);
    rt->d_mphi = std::move(phi);
    rt->d_mstate = std::move(state);
    rt->d_mring = std::move(ring);
    rt->d_mrow = std::move(row);
    rt->d_mwin = std::move(wtab);
    rt->pmap_plan = plan;
    rt->pmap_quality = quality;
    rt->pmap_max = max_nframes;
    rt->pmap_rmin = ratio_min;
    rt->pmap_rmax = ratio_max;
    if ((st = rt_pitchmap_zero(rt, nullptr)) != PV_OK || hipDeviceSynchronize() != hipSuccess) {
        rt->pmap_on = 0;
        rt->callback = rt->harm_on ? pv_rt::kHarmonPush : rt->pitch_on ? pv_rt::kPitchPush : pv_rt::kPush;
        return st != PV_OK ? st : fail(PV_ERR_HIP, f + ": zeroing the stream state");
    }
    rt->pmap_on = 1;
    rt->callback = pv_rt::kPitchmapPush;
    return PV_OK;
}

int pv_rt_pitchmap_latency(const pv_rt* rt) { return (rt && rt->pmap_on) ? rt->pmap_plan.latency : 0; }

pv_status pv_rt_pitchmap_push(pv_rt* rt, const float* in, long long ldi, int nframes, const float* ratio,
                              long long ldr, float* out, long long ldo, pv_float2* spec, long long ld_spec,
                              void* stream) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (!rt->pmap_on) return fail(PV_ERR_ARG, "pv_rt_pitchmap_push: call pv_rt_pitchmap_reserve first");
    if (nframes > rt->pmap_max)
        return fail(PV_ERR_ARG, "pv_rt_pitchmap_push: nframes > max_nframes of pv_rt_pitchmap_reserve");
    if (nframes < 0) return fail(PV_ERR_ARG, "negative nframes");
    if (nframes == 0) return PV_OK;
    pv_handle* h = rt->h;
    if (!in || !out) return fail(PV_ERR_ARG, "null in/out");
    if (rt->channels > 1 && (ldi < (long long)nframes * h->hop || ldo < (long long)nframes * h->hop))
        return fail(PV_ERR_ARG, "ldi/ldo smaller than one callback");
    if (ratio && rt->channels > 1 && ldr < nframes) return fail(PV_ERR_ARG, "ldr < nframes");
    if (spec && rt->channels > 1 && ld_spec < (long long)nframes * h->spec_stride)
        return fail(PV_ERR_ARG, "ld_spec < nframes * spec_stride");
    DeviceGuard g(h->cfg.device);
    const RtPitchmapPlan& plan = rt->pmap_plan;
    pv::RtMapParams p{};
    p.rt = rt_params(rt, in, ldi, nframes, nullptr, 0, spec, ld_spec);
    p.ratio = ratio;
    p.ldr = ldr;
    p.ratio_min = rt->pmap_rmin;
    p.ratio_max = rt->pmap_rmax;
    p.prev = rt->d_mprev;
    p.phi = rt->d_mphi;
    p.st = rt->d_mstate;
    p.ring = rt->d_mring;
    p.ring_cap = (int)plan.ring_cap;
    p.row = rt->d_mrow;
    p.ld_row = plan.row_len;
    p.K = plan.K;
    pv::RtVarParams v{};
    v.row = rt->d_mrow;
    v.ld_row = plan.row_len;
    v.K = plan.K;
    v.out = out;
    v.ldo = ldo;
    v.st = rt->d_mstate;
    v.ring = rt->d_mring;
    v.ring_cap = (int)plan.ring_cap;
    v.win = rt->d_mwin;
    v.win_scale = (float)((double)pv::kVarWinN / resample_zero_crossings(rt->pmap_quality) * 0x1p-32);
    v.channels = rt->channels;
    v.nframes = nframes;
    v.hop = h->hop;
    v.G = plan.G;
    v.rolloff = resample_rolloff(rt->pmap_quality);
    v.Z = resample_zero_crossings(rt->pmap_quality);
    hipStream_t s = (hipStream_t)stream;
    prof_tick(h);
    PV_LAUNCH(h, KRTM, s, pv::launch_rt_map(h->L_syn, rt->phase_lock, p, s));
    PV_LAUNCH(h, KRTV, s, pv::launch_rt_varresample(v, s));
    return PV_OK;
}

pv_status pv_rt_pitchmap_host_ratios(pv_rt* rt, float** host_ratio) {
    if (!rt || !rt->exec) return fail(PV_ERR_ARG, "no captured callback (pv_rt_capture)");
    if (rt->g_kind != pv_rt::kPitchmapPush)
        return fail(PV_ERR_ARG, "pv_rt_pitchmap_host_ratios: the captured callback is not pv_rt_pitchmap_push");
    if (!host_ratio) return fail(PV_ERR_ARG, "null argument");
    *host_ratio = rt->h_ratio;
    return PV_OK;
}

// ---- the captured callback
pv_status pv_rt_capture(pv_rt* rt, int nframes) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (nframes <= 0) return fail(PV_ERR_ARG, "nframes must be > 0");
    if (rt->callback == pv_rt::kPitchPush && nframes > rt->pitch_max)
        return fail(PV_ERR_ARG, "pv_rt_capture: nframes > max_nframes of pv_rt_pitch_reserve");
    if (rt->callback == pv_rt::kPitchmapPush && nframes > rt->pmap_max)
        return fail(PV_ERR_ARG, "pv_rt_capture: nframes > max_nframes of pv_rt_pitchmap_reserve");
    if (rt->callback == pv_rt::kHarmonPush && nframes > rt->harm_max)
        return fail(PV_ERR_ARG, "pv_rt_capture: nframes > max_nframes of pv_rt_harmonizer_reserve");
    pv_handle* h = rt->h;
    DeviceGuard g(h->cfg.device);
    rt_release_graph(rt);
    if (!rt->g_stream) PV_HIP(hipStreamCreateWithFlags(&rt->g_stream, hipStreamNonBlocking));
    const size_t C = (size_t)rt->channels;
    const size_t ni = (size_t)nframes * h->hop, no = (size_t)nframes * rt_out_hop(rt);
    // pinned, device-mapped host buffers: the captured kernel reads the callback's input
    // and writes its output in place over the bus (zero-copy: the graph is one kernel
    // node, two after pv_rt_pitch_reserve, pv_rt_pitchmap_reserve or pv_rt_harmonizer_reserve, no
    // copy nodes); if the runtime cannot map them, the graph copies H2D / D2H around the kernels
    // instead.  The pitch map's ratios are a third such buffer, [channels][nframes], filled with 1;
    // the harmoniser's ratios, [channels][voices][nframes], filled with 1, and its gains, a fourth
    // of the same shape, filled with 1 / voices.
    const bool with_gain = rt->callback == pv_rt::kHarmonPush;
    const bool with_ratio = with_gain || rt->callback == pv_rt::kPitchmapPush;
    const size_t nr = with_gain ? (size_t)rt->harm_voices * (size_t)nframes : with_ratio ? (size_t)nframes : 0;
    PV_HIP(rt->h_in.alloc(C * ni));
    PV_HIP(rt->h_out.alloc(C * no));
    std::memset(rt->h_in, 0, sizeof(float) * C * ni);
    std::memset(rt->h_out, 0, sizeof(float) * C * no);
    if (with_ratio) {
        PV_HIP(rt->h_ratio.alloc(C * nr));
        std::fill(rt->h_ratio.p, rt->h_ratio.p + C * nr, 1.0f);
    }
    if (with_gain) {
        PV_HIP(rt->h_gain.alloc(C * nr));
        std::fill(rt->h_gain.p, rt->h_gain.p + C * nr, 1.0f / (float)rt->harm_voices);
    }
    float *m_in = nullptr, *m_out = nullptr, *m_ratio = nullptr, *m_gain = nullptr;
    bool zero_copy = hipHostGetDevicePointer((void**)&m_in, rt->h_in, 0) == hipSuccess &&
                     hipHostGetDevicePointer((void**)&m_out, rt->h_out, 0) == hipSuccess && m_in && m_out;
    if (zero_copy && with_ratio)
        zero_copy = hipHostGetDevicePointer((void**)&m_ratio, rt->h_ratio, 0) == hipSuccess && m_ratio;
    if (zero_copy && with_gain)
        zero_copy = hipHostGetDevicePointer((void**)&m_gain, rt->h_gain, 0) == hipSuccess && m_gain;
    if (!zero_copy) {
        (void)hipGetLastError();
        PV_HIP(rt->d_in.alloc(C * ni));
        PV_HIP(rt->d_out.alloc(C * no));
        if (with_ratio) PV_HIP(rt->d_ratio.alloc(C * nr));
        if (with_gain) PV_HIP(rt->d_gain.alloc(C * nr));
    }
    hipStream_t s = rt->g_stream;
    hipGraph_t graph = nullptr;
    {
        ProfOff off(h);  // restored on every path out of the capture
        PV_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        pv_status st = PV_OK;
        if (zero_copy) {
            st = rt_callback_push(rt, m_in, (long long)ni, nframes, m_ratio, m_gain, m_out, (long long)no, s);
        } else {
            if (hipMemcpyAsync(rt->d_in, rt->h_in, sizeof(float) * C * ni, hipMemcpyHostToDevice, s) != hipSuccess ||
                (with_ratio && hipMemcpyAsync(rt->d_ratio, rt->h_ratio, sizeof(float) * C * nr, hipMemcpyHostToDevice,
                                              s) != hipSuccess) ||
                (with_gain && hipMemcpyAsync(rt->d_gain, rt->h_gain, sizeof(float) * C * nr, hipMemcpyHostToDevice,
                                             s) != hipSuccess))
                st = fail(PV_ERR_HIP, "pv_rt_capture: H2D capture failed");
            if (st == PV_OK)
                st = rt_callback_push(rt, rt->d_in, (long long)ni, nframes, rt->d_ratio, rt->d_gain, rt->d_out,
                                      (long long)no, s);
            if (st == PV_OK &&
                hipMemcpyAsync(rt->h_out, rt->d_out, sizeof(float) * C * no, hipMemcpyDeviceToHost, s) != hipSuccess)
                st = fail(PV_ERR_HIP, "pv_rt_capture: D2H capture failed");
        }
        hipError_t e = hipStreamEndCapture(s, &graph);
        if (st != PV_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return st;
        }
        if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    }
    rt->graph = graph;
    PV_HIP(hipGraphInstantiate(&rt->exec, graph, nullptr, nullptr, 0));
    rt->g_nframes = nframes;
    rt->g_kind = rt->callback;
    rt->m_in = zero_copy ? m_in : nullptr;
    rt->m_out = zero_copy ? m_out : nullptr;
    rt->m_ratio = zero_copy ? m_ratio : nullptr;
    rt->m_gain = zero_copy ? m_gain : nullptr;
    const char* lv = std::getenv("PV_RT_LAUNCH");
    rt->direct = (zero_copy && lv && std::string(lv) == "direct") ? 1 : 0;
    return PV_OK;
}

pv_status pv_rt_host_buffers(pv_rt* rt, float** host_in, float** host_out) {
    if (!rt || !rt->exec) return fail(PV_ERR_ARG, "no captured callback (pv_rt_capture)");
    if (host_in) *host_in = rt->h_in;
    if (host_out) *host_out = rt->h_out;
    return PV_OK;
}

pv_status pv_rt_callback(pv_rt* rt, const float* in, float* out) {
    if (!rt || !rt->exec) return fail(PV_ERR_ARG, "no captured callback (pv_rt_capture)");
    pv_handle* h = rt->h;
    DeviceGuard g(h->cfg.device);
    const size_t C = (size_t)rt->channels;
    const size_t ni = (size_t)rt->g_nframes * h->hop, no = (size_t)rt->g_nframes * rt_out_hop(rt);
    if (in && in != rt->h_in) std::memcpy(rt->h_in, in, sizeof(float) * C * ni);  // main.cpp:49
    if (rt->direct) {
        pv_status st = rt_callback_push(rt, rt->m_in, (long long)ni, rt->g_nframes, rt->m_ratio, rt->m_gain,
                                        rt->m_out, (long long)no, rt->g_stream);
        if (st != PV_OK) return st;
    } else {
        PV_HIP(hipGraphLaunch(rt->exec, rt->g_stream));
    }
    PV_HIP(hipStreamSynchronize(rt->g_stream));
    if (out && out != rt->h_out) std::memcpy(out, rt->h_out, sizeof(float) * C * no);
    return PV_OK;
}

}  // extern "C"
