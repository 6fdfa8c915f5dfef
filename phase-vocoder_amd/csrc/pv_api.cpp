// pv_api.cpp — host side of libpv, the C-ABI declared in include/pv.h: versions and status
// strings, pv_create / pv_destroy / pv_get_info, the table blob and the per-launch profiler.
// pv_create owns the per-handle constant tables (windows, twiddles, unwrap tables, pitch map;
// recipes: pv_tables.cpp) and the workspace (run sums, carries, overlap tails).  The other
// components are pv_api_batch.cpp (launch sequences), pv_api_rt.cpp,
// pv_api_resample.cpp and pv_api_misc.cpp.  No allocation or synchronisation happens inside
// the compute entry points, so a caller may capture them into a hipGraph.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>

#include "pv_host.hpp"

namespace pvhost {

static thread_local std::string g_last_error;

pv_status fail(pv_status s, const std::string& msg) {
    g_last_error = msg;
    return s;
}

pv_status check_common(const pv_handle* h, int channels, int frames) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    if (!h->tables_ready)
        return fail(PV_ERR_ARG, "tables_external handle: no tables yet (pv_import_tables first)");
    if (channels < 0 || frames < 0) return fail(PV_ERR_ARG, "negative channels/frames");
    if (channels > h->cfg.max_channels || frames > h->cfg.max_frames)
        return fail(PV_ERR_ARG, "channels/frames exceed the handle's capacity (max_channels, max_frames)");
    return PV_OK;
}

pv_status check_abi(const pv_config* cfg) {
    if (cfg->abi_version != PV_ABI_VERSION)
        return fail(PV_ERR_ARG, "pv_config.abi_version != PV_ABI_VERSION (caller built against another pv.h)");
    return PV_OK;
}

pv_status check_quality(const char* fn, int quality) {
    if (quality != 0 && quality != 1) return fail(PV_ERR_ARG, std::string(fn) + ": quality must be 0 (fast) or 1 (best)");
    return PV_OK;
}

pv_status check_std_stretch(const char* fn, const pv_handle* h) {
    if (h->mode != PV_MODE_STANDARD || h->effect != PV_TIME_SHIFT)
        return fail(PV_ERR_UNSUPPORTED, std::string(fn) + ": STANDARD time-stretch handles only");
    return PV_OK;
}

pv_status prof_begin_timed(pv_handle* h, int kernel, hipStream_t s) {
    hipEvent_t a, b;
    auto take = [&](hipEvent_t* e) -> pv_status {
        if (!h->prof.pool.empty()) {
            *e = h->prof.pool.back();
            h->prof.pool.pop_back();
            return PV_OK;
        }
        PV_HIP(hipEventCreate(e));
        return PV_OK;
    };
    const bool shared = h->prof.chain_ok && h->prof.chain_ev && h->prof.chain_s == s;
    pv_status st = PV_OK;
    if (shared) a = h->prof.chain_ev;
    else st = take(&a);
    if (st == PV_OK) st = take(&b);
    if (st != PV_OK) return st;
    if (!shared) PV_HIP(hipEventRecord(a, s));
    h->prof.ev_start.push_back(a);
    h->prof.ev_stop.push_back(b);
    h->prof.ev_shared.push_back(shared ? 1 : 0);
    h->prof.ev_kernel.push_back(kernel);
    return PV_OK;
}

pv_status prof_end_timed(pv_handle* h, hipStream_t s) {
    PV_HIP(hipEventRecord(h->prof.ev_stop.back(), s));
    if (h->prof.chain_ok) {
        h->prof.chain_ev = h->prof.ev_stop.back();
        h->prof.chain_s = s;
    }
    return PV_OK;
}

namespace {

// pv_create's refusals, none of which touches the device; g: the configuration's geometry
pv_status validate(const pv_config* cfg, Geometry* g) {
    pv_status st = check_abi(cfg);
    if (st != PV_OK) return st;
    const int N = cfg->n_samps;
    if (!is_pow2(N)) return fail(PV_ERR_UNSUPPORTED, "n_samps must be a power of two");
    if (cfg->mode != PV_MODE_STANDARD && cfg->mode != PV_MODE_REF_COMPAT)
        return fail(PV_ERR_ARG, "unknown mode");
    if (cfg->effect != PV_TIME_SHIFT && cfg->effect != PV_PITCH_SHIFT)
        return fail(PV_ERR_ARG, "unknown effect");
    if (cfg->hop_div <= 0 || N / cfg->hop_div <= 0) return fail(PV_ERR_ARG, "bad hop_div");
    if (cfg->max_channels < 0 || cfg->max_frames < 0) return fail(PV_ERR_ARG, "negative capacity");
    if (!(cfg->scale > 0.0f) || !std::isfinite(cfg->scale)) return fail(PV_ERR_ARG, "scale must be > 0");
    if (cfg->mode == PV_MODE_STANDARD && (N < 256 || N > 2048))
        return fail(PV_ERR_UNSUPPORTED, "STANDARD mode: n_samps in [256, 2048]");
    if (cfg->mode == PV_MODE_REF_COMPAT && (N < 256 || N > 2048))
        return fail(PV_ERR_UNSUPPORTED, "REF_COMPAT mode: n_samps in [256, 2048]");
    if (cfg->window < PV_WINDOW_DEFAULT || cfg->window > PV_WINDOW_HANN_REF)
        return fail(PV_ERR_ARG, "unknown window");
    if (cfg->mode == PV_MODE_STANDARD && cfg->window != PV_WINDOW_DEFAULT)
        return fail(PV_ERR_UNSUPPORTED, "STANDARD mode: the periodic Hann window only (window = 0)");
    if (cfg->spec_layout != PV_SPEC_NATURAL && cfg->spec_layout != PV_SPEC_PACKED)
        return fail(PV_ERR_ARG, "unknown spec_layout");
    if (cfg->spec_layout == PV_SPEC_PACKED && cfg->mode != PV_MODE_STANDARD)
        return fail(PV_ERR_UNSUPPORTED, "PV_SPEC_PACKED: STANDARD handles only");
    *g = geometry(N, cfg->hop_div, cfg->mode, cfg->effect, cfg->scale);
    if (g->hs <= 0 || g->hs > N) return fail(PV_ERR_UNSUPPORTED, "out hop must be in [1, N]");
    if (cfg->mode == PV_MODE_REF_COMPAT && cfg->effect == PV_PITCH_SHIFT && cfg->scale != 1.0f)
        return fail(PV_ERR_UNSUPPORTED, "REF_COMPAT implements no pitch shift (phaseVocoder.h:107-110)");
    // (REF_COMPAT time shift with hs != hop: kernel.cu:354 hard-codes timeScale = 1, the
    // reference only changes the OLA hop)
    if (g->L_ana > 2048 || g->L_syn > 2048 || g->L_syn < 128)
        return fail(PV_ERR_UNSUPPORTED, "FFT length outside [128, 2048]");
    return PV_OK;
}

// a constant table of the handle: uploaded, or (pv_config.tables_external) allocated zeroed
// for pv_import_tables to fill — the host copy never reaches the device
template <typename T, typename S>
pv_status upload_table(DevBuf<T>& dst, const std::vector<S>& src, bool external) {
    // (S = pv_float2 for T = float2: the recipes are written without a HIP header)
    static_assert(sizeof(S) == sizeof(T) && alignof(S) <= alignof(T), "host and device entries share a layout");
    if (external) PV_HIP(dst.alloc_zero(src.size()));
    else PV_HIP(dst.upload(reinterpret_cast<const T*>(src.data()), src.size()));
    return PV_OK;
}

// the constant tables, built on the host (pv_tables.cpp) and uploaded (pv_config.tables_external:
// allocated zeroed, filled only by pv_import_tables — a non-root rank of a multi-GPU job
// receives rank 0's)
pv_status upload_tables(pv_handle* h, const PhaseTables& pt, const PitchMap& pm) {
    const int N = h->N;
    std::vector<float> win, gain;
    if (h->mode == PV_MODE_STANDARD) {
        hann_periodic(N, win);
        std_gain(N, h->hs, gain);
    } else {
        if (h->cfg.window == PV_WINDOW_HANN_REF) hann_ref(N, win);  // PhaseVocoder(int samples)
        else hamming_ref(N, win);
        compat_gain(win, gain);
    }
    std::vector<pv_float2> tw_ana, tws_ana, tw_syn, tws_syn;
    fft_table(h->L_ana, tw_ana);
    split_twiddles(2 * h->L_ana, tws_ana);
    tw_syn_table(h->L_syn, tw_syn);
    split_twiddles(N, tws_syn);
    pv_status st = PV_OK;
    const bool ext = h->cfg.tables_external != 0;
    auto up = [&](auto& dst, const auto& src) { return (st = upload_table(dst, src, ext)) == PV_OK; };
    (void)(up(h->d_win, win) && up(h->d_gain, gain) && up(h->d_tw_ana, tw_ana) && up(h->d_tws_ana, tws_ana) &&
           up(h->d_tw_syn, tw_syn) && up(h->d_tws_syn, tws_syn) && up(h->d_ek, pt.ek) &&
           up(h->d_jk_mod, pt.jk_mod) && up(h->d_src_first, pm.first) && up(h->d_src_cnt, pm.cnt));
    return st;
}

pv_status alloc_workspace(pv_handle* h) {
    const pv_config& cfg = h->cfg;
    const int runs_fused = h->F_fused > 0 ? (cfg.max_frames + h->F_fused - 1) / h->F_fused : 0;
    const size_t chans = (size_t)std::max(cfg.max_channels, 1);
    const size_t runs_total = chans * std::max(h->max_runs, 1);
    const size_t wg_total = chans * std::max((std::max(h->max_runs, runs_fused) + 3) / 4, 1);
    if (h->mode == PV_MODE_STANDARD) {
        PV_HIP(h->d_runsum.alloc(runs_total * pv::kRecFields * h->bins_pad));
        PV_HIP(h->d_carry.alloc(runs_total * h->bins_pad));
        PV_HIP(h->d_seg_carry.alloc(chans * h->bins_pad));
        PV_HIP(h->d_seg_phi.alloc(chans * h->bins_pad));
    }
    PV_HIP(h->d_tails.alloc(wg_total * std::max(h->tail_len, 1)));
    if (h->F_fused > 0) {
        PV_HIP(h->d_seam_flags.alloc_zero(wg_total));
#ifdef PV_FUSED_STAMPS
        h->n_stamps = wg_total * 4 * pv::kFusedStampSlots;
        PV_HIP(h->d_stamps.alloc_zero(h->n_stamps));
#endif
    }
    return PV_OK;
}

struct HandleDeleter {
    void operator()(pv_handle* h) const { pv_destroy(h); }
};

}  // namespace
}  // namespace pvhost

using namespace pvhost;

extern "C" {

int pv_abi_version(void) { return PV_ABI_VERSION; }

// 2 (round 4): fused real-split accumulation, one-rounding unwrap decision (pv_device.hpp);
// 3: twiddle-first radix-E FFT passes with the window folded in, L <= 512 (fft_pass v3)
int pv_contract_version(void) { return 4; }
#ifndef PV_SOURCES_SHA
#define PV_SOURCES_SHA "unset"
#endif
const char* pv_sources_sha(void) { return PV_SOURCES_SHA; }
int pv_diagnostic_build(void) {
#ifdef PV_DIAGNOSTIC_BUILD
    return 1;
#else
    return 0;
#endif
}

const char* pv_status_string(pv_status s) {
    switch (s) {
        case PV_OK: return "PV_OK";
        case PV_ERR_ARG: return "PV_ERR_ARG";
        case PV_ERR_UNSUPPORTED: return "PV_ERR_UNSUPPORTED";
        case PV_ERR_HIP: return "PV_ERR_HIP";
        case PV_ERR_NOMEM: return "PV_ERR_NOMEM";
    }
    return "PV_ERR_UNKNOWN";
}

const char* pv_last_error(void) { return g_last_error.c_str(); }

int pv_frame_count(long long n_samples, int hop) {
    // main.cpp:231: for (i = 0; i < numSamples - hopSize; i += hopSize)
    if (hop <= 0) return 0;
    long long span = n_samples - hop;
    if (span <= 0) return 0;
    return (int)((span + hop - 1) / hop);
}

long long pv_output_length(const pv_handle* h, int frames) {
    if (!h || frames <= 0) return 0;
    return (long long)frames * h->hs + (h->N - h->hs);
}

pv_status pv_get_info(const pv_handle* h, pv_info* info) {
    if (!h || !info) return fail(PV_ERR_ARG, "null argument");
    if (info->abi_version != PV_ABI_VERSION)
        return fail(PV_ERR_ARG, "pv_info.abi_version != PV_ABI_VERSION (caller built against another pv.h)");
    info->n_samps = h->N;
    info->hop = h->hop;
    info->out_hop = h->hs;
    info->spec_bins = h->spec_bins;
    info->spec_stride = h->spec_stride;
    info->frames_per_run = h->F;
    info->mode = h->mode;
    info->effect = h->effect;
    info->scale = h->scale;
    info->single_launch = single_launch(h) ? 1 : 0;
    info->single_launch_frames = info->single_launch ? h->F_fused : 0;
    info->lane_constants = h->k_lane;
    info->spec_layout = h->packed ? PV_SPEC_PACKED : PV_SPEC_NATURAL;
    return PV_OK;
}

int pv_resident_min_channels(const pv_handle* h) { return h ? h->resident_min : 0; }

#ifdef PV_FUSED_STAMPS
// diagnostic build only (make variant NAME=stamps DEFS=-DPV_FUSED_STAMPS): the per-wave
// phase stamps of the last k_fused launch, kFusedStampSlots per wave (scripts/fused_stamps.py)
pv_status pv_debug_stamps(const pv_handle* h, unsigned long long* dst, size_t count) {
    if (!h || !dst || !h->d_stamps) return PV_ERR_ARG;
    DeviceGuard g(h->cfg.device);
    if (hipDeviceSynchronize() != hipSuccess) return PV_ERR_HIP;
    if (hipMemcpy(dst, h->d_stamps, sizeof(unsigned long long) * std::min(count, h->n_stamps),
                  hipMemcpyDeviceToHost) != hipSuccess)
        return PV_ERR_HIP;
    return PV_OK;
}
#endif

void pv_destroy(pv_handle* h) {
    if (!h) return;
    DeviceGuard g(h->cfg.device);
    pv_resampler_destroy(h->pitch_rs);
    pv_varresampler_destroy(h->pmap_vr);
    for (size_t i = 0; i < h->prof.ev_start.size(); ++i)
        if (!h->prof.ev_shared[i]) (void)hipEventDestroy(h->prof.ev_start[i]);
    for (auto e : h->prof.ev_stop) (void)hipEventDestroy(e);
    for (auto e : h->prof.pool) (void)hipEventDestroy(e);
    delete h;  // frees its tables and workspace, on its device
}

pv_status pv_create(const pv_config* cfg, pv_handle** out) {
    if (!cfg || !out) return fail(PV_ERR_ARG, "null argument");
    *out = nullptr;
    Geometry geo{};
    pv_status st = validate(cfg, &geo);
    if (st != PV_OK) return st;

    // ---- geometry
    std::unique_ptr<pv_handle, HandleDeleter> hp(new pv_handle());  // no path below leaks it
    pv_handle* h = hp.get();
    const int N = cfg->n_samps;
    h->cfg = *cfg;
    h->N = N;
    h->mode = cfg->mode;
    h->effect = cfg->effect;
    h->scale = cfg->scale;
    h->nan_faithful = (cfg->mode == PV_MODE_REF_COMPAT && cfg->nan_faithful) ? 1 : 0;
    h->hop = geo.hop;
    h->hs = geo.hs;
    h->pitch = geo.pitch;
    h->L_syn = geo.L_syn;
    h->L_ana = geo.L_ana;
    h->bins = geo.bins;
    h->bins_pad = geo.bins_pad;
    h->tail_len = geo.tail_len;
    h->packed = (cfg->spec_layout == PV_SPEC_PACKED) ? 1 : 0;
    // packed rows are exactly N/2 float2: bin N/2 rides in slot 0
    h->spec_bins = (h->mode == PV_MODE_STANDARD) ? (h->packed ? N / 2 : h->bins) : 2 * N;
    h->spec_stride = (h->spec_bins + 7) & ~7;
    h->env = read_env_overrides();

    // ---- frames per wave-run (choose_run_frames)
    const long long C = std::max(cfg->max_channels, 1), T = std::max(cfg->max_frames, 1);
    const long long work = C * T;
    int wpc = 0, W = 4;
    if (run_fit_applies(work, h->L_syn, h->L_ana, h->mode)) {
        DeviceGuard g0(cfg->device);
        wpc = pv::std_analysis_wgs_per_cu(h->L_ana, h->hop, ek_lane_of(cfg->hop_div, h->bins), h->packed != 0, &W);
    }
    h->F = choose_run_frames(work, h->L_syn, h->L_ana, h->mode, wpc, W, C, T, h->hs, h->tail_len, h->env);
    h->max_runs = (cfg->max_frames + h->F - 1) / h->F;

    // ---- tables, on the host: unwrap tables, rho = p/q, the pitch map
    PhaseTables pt;
    phase_tables(N, geo, cfg->scale, pt);
    h->rho = pt.rho;
    h->q = pt.q;
    h->p_mod = pt.p_mod;
    h->q_pow2 = pt.q_pow2;
    h->inv_q = pt.inv_q;
    if (!h->q_pow2 && pt.q > 32768) return fail(PV_ERR_UNSUPPORTED, "output-phase ratio denominator too large");
    PitchMap pm;
    pitch_map(h->bins, h->pitch != 0, cfg->scale, pm);
    h->src_hi = pm.src_hi;
    // per-lane unwrap constants (the synthesis keeps them in two registers): every bin
    // k < L repeats bin k mod 64, and bin L's e equals bin 0's (PV_SYN_LANEK=0 turns them off)
    const int smode = (h->mode == PV_MODE_REF_COMPAT) ? 1 : (h->pitch ? 2 : 0);
    h->k_lane = (bins_repeat_mod64(pt) && pv::synthesis_lane_kernel(h->L_syn, smode, h->hs, h->q_pow2 != 0, h->q) &&
                 h->env.syn_lanek)
                    ? 1
                    : 0;
    if (h->mode == PV_MODE_STANDARD && h->q == 1 && pv::fused_supported(h->L_syn, h->hs))
        h->F_fused = choose_fused_frames(h->F, work, h->hs, h->tail_len, h->env);
    {
        const ResidentGeometry rg{h->mode, h->pitch, h->L_ana, h->L_syn, h->hop, h->hs, h->q_pow2, h->k_lane,
                                  h->F, h->tail_len, h->q};
        h->resident_min = resident_min_channels(resident_supported(rg) && pv::resident_kernel(h->L_syn, h->hs), h->env);
    }

    // ---- upload, workspace
    DeviceGuard g(cfg->device);
    h->tables_ready = cfg->tables_external ? 0 : 1;
    if ((st = upload_tables(h, pt, pm)) != PV_OK) return st;
    if ((st = alloc_workspace(h)) != PV_OK) return st;
    // LDS budget check for the synthesis kernel (largest)
    size_t lds = pv::synthesis_lds_bytes(h->L_syn, h->hs);
    if (lds > 160 * 1024) return fail(PV_ERR_UNSUPPORTED, "LDS budget exceeded");
    *out = hp.release();
    return PV_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- table blob
namespace {
struct TableBlobHeader {
    uint32_t magic, version;
    int32_t n_samps, hop, hs, mode, effect, pitch;
    float scale;
    int32_t L_ana, L_syn, bins;
    uint32_t pad[4];
};
static_assert(sizeof(TableBlobHeader) == 64, "blob header is 64 bytes");
constexpr uint32_t kBlobMagic = 0x50565442u;  // "PVTB"

struct TableSeg {
    void* ptr;
    size_t bytes;
};
std::vector<TableSeg> table_segments(const pv_handle* h) {
    const size_t N = h->N, B = h->bins;
    return {{h->d_win.p, sizeof(float) * N},
            {h->d_gain.p, sizeof(float) * N},
            {h->d_tw_ana.p, sizeof(float2) * h->L_ana},
            {h->d_tws_ana.p, sizeof(float2) * (h->L_ana + 1)},
            {h->d_tw_syn.p, sizeof(float2) * tw_syn_len(h->L_syn)},
            {h->d_tws_syn.p, sizeof(float2) * (N / 2 + 1)},
            {h->d_ek.p, sizeof(float) * B},
            {h->d_jk_mod.p, sizeof(unsigned) * B},
            {h->d_src_first.p, sizeof(int) * B},
            {h->d_src_cnt.p, sizeof(int) * B}};
}
TableBlobHeader blob_header(const pv_handle* h) {
    TableBlobHeader hd{};
    hd.magic = kBlobMagic;
    hd.version = 2;  // 2: the L/2 synthesis table only at L = 256, 512 (tw_syn_len)
    hd.n_samps = h->N;
    hd.hop = h->hop;
    hd.hs = h->hs;
    hd.mode = h->mode;
    hd.effect = h->effect;
    hd.pitch = h->pitch;
    hd.scale = h->scale;
    hd.L_ana = h->L_ana;
    hd.L_syn = h->L_syn;
    hd.bins = h->bins;
    return hd;
}
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

extern "C" {

pv_status pv_export_tables(const pv_handle* h, void* dst, size_t cap, size_t* bytes, void* stream) {
    if (!h || !bytes) return fail(PV_ERR_ARG, "null argument");
    if (dst && !h->tables_ready) return fail(PV_ERR_ARG, "tables_external handle: no tables to export yet");
    size_t total = sizeof(TableBlobHeader);
    for (const auto& sg : table_segments(h)) total += align16(sg.bytes);
    *bytes = total;
    if (!dst) return PV_OK;
    if (cap < total) return fail(PV_ERR_ARG, "export buffer too small");
    DeviceGuard g(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    static thread_local TableBlobHeader hd;  // host source must outlive the async copy
    hd = blob_header(h);
    PV_HIP(hipMemcpyAsync(dst, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    size_t off = sizeof(TableBlobHeader);
    for (const auto& sg : table_segments(h)) {
        PV_HIP(hipMemcpyAsync((char*)dst + off, sg.ptr, sg.bytes, hipMemcpyDeviceToDevice, s));
        off += align16(sg.bytes);
    }
    PV_HIP(hipStreamSynchronize(s));
    return PV_OK;
}

pv_status pv_import_tables(pv_handle* h, const void* src, size_t bytes, void* stream) {
    if (!h || !src) return fail(PV_ERR_ARG, "null argument");
    size_t total = 0;
    pv_export_tables(h, nullptr, 0, &total, nullptr);
    if (bytes != total) return fail(PV_ERR_ARG, "table blob size does not match this handle");
    DeviceGuard g(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    TableBlobHeader hd{};
    PV_HIP(hipMemcpyAsync(&hd, src, sizeof(hd), hipMemcpyDeviceToHost, s));
    PV_HIP(hipStreamSynchronize(s));
    TableBlobHeader mine = blob_header(h);
    if (std::memcmp(&hd, &mine, sizeof(hd)) != 0)
        return fail(PV_ERR_ARG, "table blob was built for a different configuration");
    size_t off = sizeof(TableBlobHeader);
    for (const auto& sg : table_segments(h)) {
        PV_HIP(hipMemcpyAsync(sg.ptr, (const char*)src + off, sg.bytes, hipMemcpyDeviceToDevice, s));
        off += align16(sg.bytes);
    }
    PV_HIP(hipStreamSynchronize(s));
    h->tables_ready = 1;
    return PV_OK;
}

pv_status pv_set_window(pv_handle* h, const float* win, void* stream) {
    if (!h || !win) return fail(PV_ERR_ARG, "null argument");
    if (h->mode != PV_MODE_REF_COMPAT)
        return fail(PV_ERR_UNSUPPORTED, "pv_set_window: REF_COMPAT handles only");
    DeviceGuard g(h->cfg.device);
    hipError_t e = pv::launch_window_gain(win, h->d_win, h->d_gain, h->N, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("pv_set_window: ") + hipGetErrorString(e));
    return PV_OK;
}

pv_status pv_test_overlap_add(const float* in, const float* win, const float* back, float* out,
                              int n, int hop, void* stream) {
    if (!in || !win || !back || !out || n <= 0 || hop < 0) return fail(PV_ERR_ARG, "bad argument");
    hipError_t e = pv::launch_overlap_test(in, win, back, out, n, hop, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("test_overlap_add: ") + hipGetErrorString(e));
    return PV_OK;
}

// ---------------------------------------------------------------- profiler
pv_status pv_profile_enable(pv_handle* h, int enable) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    if (enable < 0) return fail(PV_ERR_ARG, "negative profile stride");
    h->prof.enabled = enable != 0;
    h->prof.stride = enable > 1 ? enable : 1;
    h->prof.calls = 0;
    h->prof.active = true;
    if (h->prof.enabled) {  // events for the first launches, created here, not per launch
        DeviceGuard g(h->cfg.device);
        while (h->prof.pool.size() < 512) {
            hipEvent_t e;
            PV_HIP(hipEventCreate(&e));
            h->prof.pool.push_back(e);
        }
    }
    return PV_OK;
}

int pv_profile_read(pv_handle* h, const char** names, double* total_ms, int* launches, int cap) {
    if (!h) return 0;
    DeviceGuard g(h->cfg.device);
    for (size_t i = 0; i < h->prof.ev_start.size(); ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(h->prof.ev_stop[i]) == hipSuccess &&
            hipEventElapsedTime(&ms, h->prof.ev_start[i], h->prof.ev_stop[i]) == hipSuccess) {
            h->prof.total_ms[h->prof.ev_kernel[i]] += ms;
            h->prof.launches[h->prof.ev_kernel[i]] += 1;
        }
        if (!h->prof.ev_shared[i]) h->prof.pool.push_back(h->prof.ev_start[i]);
        h->prof.pool.push_back(h->prof.ev_stop[i]);
    }
    h->prof.ev_start.clear();
    h->prof.ev_stop.clear();
    h->prof.ev_shared.clear();
    h->prof.ev_kernel.clear();
    h->prof.chain_ev = nullptr;
    int n = 0;
    for (int k = 0; k < kNumKernels && n < cap; ++k) {
        if (h->prof.launches[k] == 0) continue;
        if (names) names[n] = kKernelNames[k];
        if (total_ms) total_ms[n] = h->prof.total_ms[k];
        if (launches) launches[n] = h->prof.launches[k];
        ++n;
    }
    return n;
}

void pv_profile_reset(pv_handle* h) {
    if (!h) return;
    (void)pv_profile_read(h, nullptr, nullptr, nullptr, 0);
    for (int k = 0; k < kNumKernels; ++k) {
        h->prof.total_ms[k] = 0;
        h->prof.launches[k] = 0;
    }
}

}  // extern "C"
