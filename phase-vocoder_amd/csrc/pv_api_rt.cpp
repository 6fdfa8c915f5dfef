// pv_api_rt.cpp — real-time mode of libpv: pv_rt (pv_host.hpp) is a pv_handle (tables) +
// per-channel stream state + an optional captured graph of one callback (pinned host in ->
// device -> pv_rt_push -> pinned host out); the real-time pitch shift adds the locked stretch
// and the streaming resampler.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "pv_host.hpp"

using namespace pvhost;

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
    rt->g_nframes = 0;
}
// samples per frame a callback emits: hop once pv_rt_pitch_reserve has succeeded, else out hop
int rt_out_hop(const pv_rt* rt) { return rt->pitch_on ? rt->h->hop : rt->h->hs; }
// what a callback runs: pv_rt_pitch_push after pv_rt_pitch_reserve, else pv_rt_push
pv_status rt_callback_push(pv_rt* rt, const float* in, long long ldi, int nframes, float* out, long long ldo,
                           hipStream_t s) {
    return rt->pitch_on ? pv_rt_pitch_push(rt, in, ldi, nframes, out, ldo, nullptr, 0, s)
                        : pv_rt_push(rt, in, ldi, nframes, out, ldo, nullptr, 0, s);
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

// ---- the captured callback
pv_status pv_rt_capture(pv_rt* rt, int nframes) {
    if (!rt) return fail(PV_ERR_ARG, "null rt");
    if (nframes <= 0) return fail(PV_ERR_ARG, "nframes must be > 0");
    if (rt->pitch_on && nframes > rt->pitch_max)
        return fail(PV_ERR_ARG, "pv_rt_capture: nframes > max_nframes of pv_rt_pitch_reserve");
    pv_handle* h = rt->h;
    DeviceGuard g(h->cfg.device);
    rt_release_graph(rt);
    if (!rt->g_stream) PV_HIP(hipStreamCreateWithFlags(&rt->g_stream, hipStreamNonBlocking));
    const size_t C = (size_t)rt->channels;
    const size_t ni = (size_t)nframes * h->hop, no = (size_t)nframes * rt_out_hop(rt);
    // pinned, device-mapped host buffers: the captured kernel reads the callback's input
    // and writes its output in place over the bus (zero-copy: the graph is one kernel
    // node, two after pv_rt_pitch_reserve, no copy nodes); if the runtime cannot map them,
    // the graph copies H2D / D2H around the kernels instead
    PV_HIP(rt->h_in.alloc(C * ni));
    PV_HIP(rt->h_out.alloc(C * no));
    std::memset(rt->h_in, 0, sizeof(float) * C * ni);
    std::memset(rt->h_out, 0, sizeof(float) * C * no);
    float *m_in = nullptr, *m_out = nullptr;
    bool zero_copy = hipHostGetDevicePointer((void**)&m_in, rt->h_in, 0) == hipSuccess &&
                     hipHostGetDevicePointer((void**)&m_out, rt->h_out, 0) == hipSuccess && m_in && m_out;
    if (!zero_copy) {
        (void)hipGetLastError();
        PV_HIP(rt->d_in.alloc(C * ni));
        PV_HIP(rt->d_out.alloc(C * no));
    }
    hipStream_t s = rt->g_stream;
    hipGraph_t graph = nullptr;
    {
        ProfOff off(h);  // restored on every path out of the capture
        PV_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        pv_status st = PV_OK;
        if (zero_copy) {
            st = rt_callback_push(rt, m_in, (long long)ni, nframes, m_out, (long long)no, s);
        } else {
            if (hipMemcpyAsync(rt->d_in, rt->h_in, sizeof(float) * C * ni, hipMemcpyHostToDevice, s) != hipSuccess)
                st = fail(PV_ERR_HIP, "pv_rt_capture: H2D capture failed");
            if (st == PV_OK)
                st = rt_callback_push(rt, rt->d_in, (long long)ni, nframes, rt->d_out, (long long)no, s);
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
    rt->m_in = zero_copy ? m_in : nullptr;
    rt->m_out = zero_copy ? m_out : nullptr;
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
        pv_status st = rt_callback_push(rt, rt->m_in, (long long)ni, rt->g_nframes, rt->m_out, (long long)no,
                                        rt->g_stream);
        if (st != PV_OK) return st;
    } else {
        PV_HIP(hipGraphLaunch(rt->exec, rt->g_stream));
    }
    PV_HIP(hipStreamSynchronize(rt->g_stream));
    if (out && out != rt->h_out) std::memcpy(out, rt->h_out, sizeof(float) * C * no);
    return PV_OK;
}

}  // extern "C"
