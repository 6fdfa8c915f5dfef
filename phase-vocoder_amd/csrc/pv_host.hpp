// pv_host.hpp — what the host translation units of libpv share (pv_api*.cpp): error
// reporting, the device-memory owner, the handle structs, the per-launch profiler and the
// launch sequences one component calls of another.  Nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/pv.h"
#include "pv_kernels.h"
#include "pv_pitchtrack.hpp"
#include "pv_resample.hpp"
#include "pv_tables.hpp"
#include "pv_varresample.hpp"

#pragma GCC visibility push(hidden)
namespace pvhost {

using namespace pvtab;

// records the calling thread's pv_last_error() (pv_api.cpp) and returns s
pv_status fail(pv_status s, const std::string& msg);

#define PV_HIP(expr)                                                                    \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(e_ == hipErrorOutOfMemory ? PV_ERR_NOMEM : PV_ERR_HIP,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// kernel ids of the per-launch profile and their names (pv_profile_read), index for index
enum { KA, KRS, KC, KS, KSEAM, KCA, KRT, KF, KSL, KENV, KSF, KRES, KRTR, KSW, KON, KPK, KRST, KSR, KMS, KMC, KSM,
       KVR, KRD, KPT, KRTM, KRTV, KRTH, KRTHR, kNumKernels };
inline constexpr const char* kKernelNames[] = {"analysis", "runsum", "carry", "synthesis", "seam",
                                               "compat_analysis", "rt", "fused", "synthesis_locked",
                                               "envelope", "synthesis_formant", "resample", "rt_resample",
                                               "synthesis_warp", "onset", "pick", "reset", "synthesis_reset",
                                               "map_sum", "map_carry", "synthesis_map", "var_resample",
                                               "resident", "pitch", "rt_map", "rt_varresample",
                                               "rt_hmap", "rt_hresample"};
static_assert(sizeof(kKernelNames) / sizeof(kKernelNames[0]) == kNumKernels, "one name per kernel id");

// Move-only owner of one hipMalloc (Pinned: hipHostMalloc, device-mapped) allocation.  Converts
// to the raw pointer kernels receive; freed on reset() or destruction, on the device that is
// current then (callers hold a DeviceGuard).
template <typename T, bool Pinned = false>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void reset() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
    }
    // n elements (at least one byte is allocated); the earlier allocation is released first
    hipError_t alloc(size_t n) {
        reset();
        const size_t bytes = sizeof(T) * (n ? n : 1);
        hipError_t e = Pinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocMapped) : hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    hipError_t alloc_zero(size_t n) {
        hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(p, 0, sizeof(T) * (n ? n : 1));
    }
    hipError_t upload(const T* src, size_t n) {
        hipError_t e = alloc(n);
        return (e != hipSuccess || n == 0) ? e : hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice);
    }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct Profile {
    bool enabled = false;
    int stride = 1;        // time every stride-th pv_analysis / pv_resynthesis / pv_process call
    long long calls = 0;
    bool active = true;    // this call's launches are timed
    // consecutive launches of one call share an event: launch i's stop is launch i+1's start
    // (nothing else is enqueued between them), one event record per launch instead of two
    bool chain_ok = false;
    hipEvent_t chain_ev = nullptr;
    hipStream_t chain_s = nullptr;
    std::vector<hipEvent_t> ev_start, ev_stop;
    std::vector<char> ev_shared;   // ev_start[i] is ev_stop[i-1] (returned to the pool once)
    std::vector<hipEvent_t> pool;  // read-out events, reused (hipEventCreate per launch costs µs)
    std::vector<int> ev_kernel;
    double total_ms[kNumKernels] = {0};
    int launches[kNumKernels] = {0};
};

}  // namespace pvhost

struct pv_handle {
    pv_config cfg{};
    int N = 0, hop = 0, hs = 0, L_ana = 0, L_syn = 0, bins = 0, bins_pad = 0;
    int spec_bins = 0, spec_stride = 0, F = 16, tail_len = 0, max_runs = 0;
    int F_fused = 0;  // frames per run of the single-launch q = 1 path (0: not available)
    int resident_min = 0;  // channels from which a spec = NULL call takes k_resident (0: never)
    pvtab::EnvOverrides env;  // environment overrides, read once by pv_create (pv.h lists them)
    int src_hi = 0;   // highest analysis bin any output bin reads (pitch map; L otherwise)
    int tables_ready = 1;  // 0: pv_config.tables_external until pv_import_tables
    int mode = 0, effect = 0, pitch = 0, aligned_hop = 1, nan_faithful = 0;
    int packed = 0;  // PV_SPEC_PACKED rows (STANDARD)
    int phase_lock = 0;  // pv_set_phase_lock: identity phase locking (k_synthesis in the locked mode)
    // pv_set_formant: lifter order of the formant-preserving pitch shift (0: off), and the
    // handle's envelope rows [max_channels][max_frames][env_stride] fp32 (allocated once, zeroed;
    // a harmoniser's voices read voice 0's)
    int formant = 0;
    int env_stride = 0;
    pvhost::DevBuf<float> d_env;
    // pv_pitch_set_formant: lifter order of the envelope warp of the time stretch (0: off; the
    // rows are d_env), and the warp map {i_k}, {bits of f_k} for k <= N/2 (pvtab::warp_map)
    int pitch_formant = 0;
    pvhost::DevBuf<int> d_warp_idx, d_warp_frac;
    // pv_pitch_reserve: the resampler of pv_pitch_process (P = out hop, Q = hop) and the scratch
    // rows the time stretch writes for it, [max_channels][ld_pitch] fp32
    pv_resampler* pitch_rs = nullptr;
    pvhost::DevBuf<float> d_pitch;
    long long ld_pitch = 0;
    // pv_set_transient: the transient phase reset of the time stretch (PV_TRANSIENT_*), the
    // detector's threshold, and the buffers of pv_transient_reserve (allocated once, zeroed):
    // flags [max_channels][max_frames] bytes, {rise, tot} [max_channels][max_frames], Theta
    // [max_channels][max_runs][bins_pad], prev_reset_run [max_channels][max_runs]
    int transient = 0;
    float transient_thr = PV_TRANSIENT_DEFAULT_THRESHOLD;
    pvhost::DevBuf<unsigned char> d_tr_flags;
    pvhost::DevBuf<float2> d_tr_strength;
    pvhost::DevBuf<float> d_tr_theta;
    pvhost::DevBuf<int> d_tr_prr;
    std::mutex tr_mu;
    // pv_timemap_set: the time map {i_u, a_u} of pv_timemap_process (max_frames entries), its
    // length (0: no map) and highest row index, and the integer phase scan's run sums and
    // carries, [max_channels][max_runs][bins_pad] each (allocated by the first set, zeroed)
    int map_n = 0, map_imax = 0;
    pvhost::DevBuf<pv::MapEntry> d_map;
    // pv_timemap_set_channels: a map per channel (map_channels > 0; 0: the shared map or none).
    // d_map then holds max_channels rows of max_frames entries (grown by the first such set),
    // d_map_counts the channels' frame counts (passed to the kernels only when one is below
    // map_n: map_counted); map_imax_c the highest row index of each channel's counted frames.
    int map_channels = 0, map_counted = 0;
    long long map_rows = 0;  // rows of max_frames entries d_map holds (1: the shared map only)
    pvhost::DevBuf<int> d_map_counts;
    std::vector<int> map_imax_c;
    pvhost::DevBuf<unsigned> d_map_sum, d_map_carry;
    // pv_pitchmap_set: the variable-rate resampler of pv_pitchmap_process (blocks of hop samples)
    // and the final frames n of the pitch map (0: no pitch map; the time map is then the
    // caller's).  The stretch writes the scratch rows of pv_pitch_process, d_pitch.
    pv_varresampler* pmap_vr = nullptr;
    int pmap_n = 0;
    float scale = 1.0f, rho = 1.0f, inv_q = 1.0f;
    unsigned long long p_mod = 0, q = 1;
    int q_pow2 = 1;
    int k_lane = 0;  // e_k and (p j_k) mod q depend on k mod 64 only (synthesis LANEK kernels)
    // device tables
    pvhost::DevBuf<float> d_win, d_gain, d_ek;
    pvhost::DevBuf<float2> d_tw_ana, d_tws_ana, d_tw_syn, d_tws_syn;
    pvhost::DevBuf<unsigned> d_jk_mod;
    pvhost::DevBuf<int> d_src_first, d_src_cnt;
    // workspace
    pvhost::DevBuf<int> d_runsum, d_carry;
    pvhost::DevBuf<int> d_seg_carry;  // [C][bins_pad] unwrap count before a stream segment
    pvhost::DevBuf<float> d_seg_phi;  // [C][bins_pad] phase of the frame before it
    pvhost::DevBuf<float> d_tails;
    // pv_process without a spectrum buffer on the split path: the handle's own rows
    // (max_channels x max_frames, zeroed; allocated by pv_reserve_spectrum or the first such
    // call outside a stream capture — spec_mu orders concurrent first calls)
    pvhost::DevBuf<pv_float2> d_spec_own;
    std::mutex spec_mu;
    pvhost::DevBuf<int> d_seam_flags;  // fused path: per (channel, workgroup) arrival counters
#ifdef PV_FUSED_STAMPS
    pvhost::DevBuf<unsigned long long> d_stamps;  // diagnostic build: per-wave phase stamps of k_fused
    size_t n_stamps = 0;
#endif
    pvhost::Profile prof;
};

// pv_rt: a pv_handle (tables) + per-channel stream state + an optional captured graph
// of one callback (pinned host in -> device -> pv_rt_push -> pinned host out).
struct pv_rt {
    pv_handle* h = nullptr;
    int channels = 0;
    pvhost::DevBuf<float> d_hist, d_ola, d_phprev;
    pvhost::DevBuf<int> d_M;
    pvhost::DevBuf<unsigned> d_tcount;
    int phase_lock = 0;  // pv_rt_set_phase_lock: k_rt in kModeLocked
    // pv_rt_pitch_reserve: the streaming resampler of pv_rt_pitch_push (P = out hop, Q = hop,
    // reduced).  d_prow: [channels][ld_prow] scratch rows [H history | max_nframes * out hop new
    // stretched samples]; d_ptab: [Q][2W] coefficients (nullptr at ratio 1: no resampling)
    int pitch_on = 0, pitch_P = 1, pitch_Q = 1, pitch_W = 0, pitch_H = 0, pitch_D = 0, pitch_max = 0;
    pvhost::DevBuf<float> d_prow, d_ptab;
    long long ld_prow = 0;
    // pv_rt_pitchmap_reserve: the real-time pitch map's preset, ratio range and
    // plan, and its stream state per channel: d_mprev [bins_pad] the last analysed row {mag, bits
    // of P}, d_mphi [bins_pad] Phi, d_mstate, d_mring [ring_cap] the steps not yet emitted, d_mrow
    // [row_len] the scratch row [K history | final stretched samples]; d_mwin: the window table
    int pmap_on = 0, pmap_quality = 0, pmap_max = 0;
    float pmap_rmin = 1.0f, pmap_rmax = 1.0f;
    pvtab::RtPitchmapPlan pmap_plan{};
    pvhost::DevBuf<float2> d_mprev, d_mwin;
    pvhost::DevBuf<unsigned> d_mphi;
    pvhost::DevBuf<pv::RtMapState> d_mstate;
    pvhost::DevBuf<long long> d_mring;
    pvhost::DevBuf<float> d_mrow;
    // pv_rt_harmonizer_reserve: the real-time harmoniser's voices, preset, ratio
    // range and plan (the pitch map's, per voice), and its stream state: per channel d_hprev
    // [bins_pad] the last analysed row (the input history is d_hist); per (channel, voice) d_hphi
    // [bins_pad], d_hola [N] the overlap accumulator, d_hstate, d_hring [ring_cap] {step, gain},
    // d_hrow [row_len], d_hgprev the last emitted gain; d_hwin: the window table
    int harm_on = 0, harm_voices = 0, harm_quality = 0, harm_max = 0;
    float harm_rmin = 1.0f, harm_rmax = 1.0f;
    pvtab::RtPitchmapPlan harm_plan{};
    pvhost::DevBuf<float2> d_hprev, d_hwin;
    pvhost::DevBuf<unsigned> d_hphi;
    pvhost::DevBuf<float> d_hola, d_hrow;
    pvhost::DevBuf<pv::RtMapState> d_hstate;
    pvhost::DevBuf<pv::RtHStep> d_hring;
    pvhost::DevBuf<pv::RtHGain> d_hgprev;
    // what pv_rt_capture records: the later successful reserve decides
    enum { kPush = 0, kPitchPush = 1, kPitchmapPush = 2, kHarmonPush = 3 };
    int callback = kPush;
    // captured callback: g_kind is the `callback` it recorded.  h_ratio / d_ratio / m_ratio: the
    // ratios of a captured pv_rt_pitchmap_push, [channels][g_nframes], or of a captured
    // pv_rt_harmonizer_push, [channels][voices][g_nframes], whose gains are h_gain / d_gain / m_gain
    int g_nframes = 0, g_kind = kPush;
    pvhost::DevBuf<float, true> h_in, h_out, h_ratio, h_gain;
    pvhost::DevBuf<float> d_in, d_out, d_ratio, d_gain;
    float *m_ratio = nullptr, *m_gain = nullptr;
    hipStream_t g_stream = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    float *m_in = nullptr, *m_out = nullptr;  // device views of h_in / h_out (zero-copy)
    int direct = 0;  // PV_RT_LAUNCH=direct: launch pv_rt_push per callback instead of replaying
                     // the captured graph (BASELINE config 5's form, the default): measured p50
                     // 21 vs 28 us per callback on ROCm 7.2
};

// pv_resampler: a reduced ratio P:Q, a quality preset and the polyphase coefficient table in
// device memory (pv_resample.hpp)
struct pv_resampler {
    int P = 1, Q = 1, quality = 0, device = 0;
    pv::ResamplePlan plan{};
    pvhost::DevBuf<float4> d_tab;  // nullptr at ratio 1: the rows are copied
};

// pv_varresampler: a quality preset, the block length and the device records of the current map
// (pv_varresample.hpp)
struct pv_varresampler {
    int quality = 0, block = 0, max_blocks = 0, device = 0;
    int nblocks = 0;        // 0: no map
    int copy = 0;           // every step 2^32, no fraction: the rows shifted by copy_shift samples
    long long copy_shift = 0;
    int span4_max = 0;      // the largest staged span of the map's tiles (over the channels)
    pvhost::DevBuf<pv::VarBlock> d_blocks;  // [max_blocks], zeroed
    pvhost::DevBuf<pv::VarTile> d_tiles;    // [ceil(max_blocks block / kVarTile)], zeroed
    // pv_varresampler_set_maps: records per channel (map_channels > 0; 0: the shared map or none),
    // [cap_channels][max_blocks] and [cap_channels][tiles as above], and per channel the shift of
    // a channel that is a copy (every step 2^32, no fraction in its start), -1 for a filtered one;
    // copy != 0 then says that every channel is a copy
    int map_channels = 0, cap_channels = 0;
    pvhost::DevBuf<pv::VarBlock> d_blocks_c;
    pvhost::DevBuf<pv::VarTile> d_tiles_c;
    pvhost::DevBuf<long long> d_shift_c;
    pvhost::DevBuf<float2> d_win;           // [kVarWinN + 1]
};

namespace pvhost {

// ---- profiler (pv_api.cpp)
// one public call (pv_analysis / pv_resynthesis / pv_process / pv_rt_push): with a stride k > 1 only every
// k-th call's launches get events (each event record costs the queue a few us, which a
// 40-us single-stream step would otherwise carry in its timed region)
inline void prof_tick(pv_handle* h) {
    if (h->prof.enabled) h->prof.active = (h->prof.calls++ % h->prof.stride) == 0;
}
// the event records around a timed launch; untimed launches pay two tests, inline
pv_status prof_begin_timed(pv_handle* h, int kernel, hipStream_t s);
pv_status prof_end_timed(pv_handle* h, hipStream_t s);
inline bool prof_timed(const pv_handle* h) { return h->prof.enabled && h->prof.active; }
inline pv_status prof_begin(pv_handle* h, int kernel, hipStream_t s) {
    return prof_timed(h) ? prof_begin_timed(h, kernel, s) : PV_OK;
}
inline pv_status prof_end(pv_handle* h, hipStream_t s) { return prof_timed(h) ? prof_end_timed(h, s) : PV_OK; }

// the launches of one pv_analysis / pv_resynthesis / pv_process call, which enqueue nothing
// but kernels, may chain their events
struct ProfCall {
    pv_handle* h;
    explicit ProfCall(pv_handle* hh) : h(hh) {
        prof_tick(h);
        h->prof.chain_ok = true;
        h->prof.chain_ev = nullptr;
    }
    ~ProfCall() { h->prof.chain_ok = false; h->prof.chain_ev = nullptr; }
};

#define PV_LAUNCH(h, kid, s, call)                                                    \
    do {                                                                              \
        pv_status st_ = prof_begin(h, kid, s);                                        \
        if (st_ != PV_OK) return st_;                                                 \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess)                                                         \
            return fail(PV_ERR_HIP, std::string(kKernelNames[kid]) + " launch: " +    \
                                        hipGetErrorString(e_));                       \
        st_ = prof_end(h, s);                                                         \
        if (st_ != PV_OK) return st_;                                                 \
    } while (0)

// ---- checks several entry points share (pv_api.cpp)
pv_status check_common(const pv_handle* h, int channels, int frames);
// a caller's pv_config was built against this pv.h: checked before any other field is read
pv_status check_abi(const pv_config* cfg);
// "<fn>: quality must be 0 (fast) or 1 (best)"
pv_status check_quality(const char* fn, int quality);
// "<fn>: STANDARD time-stretch handles only"
pv_status check_std_stretch(const char* fn, const pv_handle* h);

inline int nruns_of(const pv_handle* h, int frames) { return (frames + h->F - 1) / h->F; }
// the caller's spectrum rows hold `frames` frames
inline pv_status check_ld_spec(const pv_handle* h, int frames, long long ld_spec) {
    if (ld_spec < (long long)frames * h->spec_stride) return fail(PV_ERR_ARG, "ld_spec < frames * spec_stride");
    return PV_OK;
}
// the v3 pass table of the batched synthesis's inverse FFT (tw_syn_table: the second block at
// L = 1024, the first otherwise)
inline const float2* syn_v3_table(const pv_handle* h) { return h->d_tw_syn + (h->L_syn == 1024 ? h->L_syn : 0); }
// the analysis keeps e_k in a register per lane (k_std_analysis EK_LANE)
inline bool ek_lane_of(int hop_div, int bins) { return 64 % hop_div == 0 && bins >= 64; }
// the single launch serves the handle's pv_process calls (phase locking, formant preservation,
// the envelope warp and the transient phase reset run on the split path)
inline bool single_launch(const pv_handle* h) {
    return h->F_fused > 0 && !h->phase_lock && !h->formant && !h->pitch_formant && !h->transient;
}

// ---- launch sequences (pv_api_batch.cpp)
// the state before a segment of a longer stream (pv_segment_resynthesis)
struct SegState {
    const int* carry_in;
    const float* phi_in;
    unsigned t_off;
};
pv_status do_analysis(pv_handle* h, const float* x, long long ldx, long long n, int C, int frames,
                      pv_float2* spec, long long ld_spec, bool want_runsum, hipStream_t s, int src_hi = -1);
pv_status do_envelope(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames, int order,
                      float* env, long long ld_env, int env_stride, int env_tail, hipStream_t s);
pv_status do_resynthesis(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames,
                         const float* ola_in, long long ld_ola, float* out, long long ldo, bool have_runsum,
                         hipStream_t s, const int* carry_from = nullptr, bool force_scan = false,
                         const SegState* seg = nullptr, const float* env_from = nullptr);
pv_status do_fused(pv_handle* h, const float* x, long long ldx, long long n, int C, int frames, pv_float2* spec,
                   long long ld_spec, float* out, long long ldo, hipStream_t s);
// the channel-resident launch (pv_resident.hip) of a spec = NULL call: out equal to
// do_analysis + do_resynthesis bit for bit, no spectrum rows anywhere
pv_status do_resident(pv_handle* h, const float* x, long long ldx, long long n, int C, int frames, float* out,
                      long long ldo, hipStream_t s);
// pv_process after its checks (the caller holds the device guard and the profile call)
pv_status process_impl(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels, int frames,
                       pv_float2* spec, long long ld_spec, float* out, long long ldo, hipStream_t s);
// the parts of do_resynthesis and process_impl that pv_timemap_process shares: the synthesis
// arguments every mode starts from, the seam launch, the handle's own rows of a spec = NULL call
pv::SynParams syn_params(const pv_handle* h, const pv_float2* spec, long long ld_spec, int frames, float* out,
                         long long ldo, long long olen);
pv_status do_seam(pv_handle* h, int C, int frames, const float* ola_in, long long ld_ola, float* out, long long ldo,
                  long long olen, hipStream_t s);
pv_status own_spectrum(pv_handle* h, const char* fn, hipStream_t s, pv_float2** spec, long long* ld_spec);
// own_rows: allocate the handle's envelope rows (a harmoniser's voices k > 0 read voice 0's)
pv_status set_formant(pv_handle* h, int order, bool own_rows);

// ---- real-time mode (pv_api_rt.cpp): k_rt's parameter block (pv_rt_push; the stretches of
// pv_rt_pitchmap_push and pv_rt_harmonizer_push read the same fields)
pv::RtParams rt_params(const pv_rt* rt, const float* in, long long ldi, int nframes, float* out, long long ldo,
                       pv_float2* spec, long long ld_spec);
// ---- real-time harmoniser (pv_api_rt_harmon.cpp): its stream state, zeroed (a stream's start)
pv_status rt_harmon_zero(pv_rt* rt, hipStream_t s);

// ---- transient phase reset (pv_api_transient.cpp)
// the handle's transient buffers exist, or are allocated now (refused while s is being captured)
pv_status transient_ready(pv_handle* h, const char* fn, hipStream_t s);
// do_resynthesis with the feature on: before the carries, the flags (k_onset + k_pick, or
// k_pick's run scan on the caller's flags) ...
pv_status transient_flags(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames, hipStream_t s);
// ... and after them, Theta of the flagged runs (k_reset) and the reset fields of the synthesis
pv_status transient_offsets(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames,
                            const int* carry, pv::SynParams* p, hipStream_t s);

// ---- resampler (pv_api_resample.cpp)
// the launch of pv_resample / pv_pitch_process (arguments checked by the caller)
hipError_t resample_rows(const pv_resampler* rs, const float* x, long long ldx, long long n_in, int channels,
                         float* y, long long ldy, hipStream_t s);

// ---- time map (pv_api_timemap.cpp): pv_timemap_set and pv_timemap_process under the name of
// the entry point that calls them (pv_pitchmap_set installs its stretch map through the first;
// pv_pitchmap_process runs the second into the scratch rows): the handle's kind, the refusals of a
// call with channels > 0, and the launches (the caller holds the device guard and the profile call)
pv_status timemap_set(const char* fn, pv_handle* h, const double* pos, int n_out);
// pv_timemap_set_channels (pv_pitchmap_set_channels installs its stretch maps through it)
pv_status timemap_set_channels(const char* fn, pv_handle* h, const double* pos, long long ld_pos, const int* counts,
                               int channels, int n_out);
pv_status timemap_handle_check(const char* fn, const pv_handle* h);
pv_status timemap_check(const char* fn, const pv_handle* h, const float* x, int channels, int frames,
                        const float* out, long long ldo);
pv_status timemap_launch(const char* fn, pv_handle* h, const float* x, long long ldx, long long n_samples,
                         int channels, int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                         hipStream_t s);

// ---- variable-rate resampler (pv_api_varresample.cpp)
// the launch of pv_varresample / pv_pitchmap_process (arguments checked by the caller)
hipError_t varresample_rows(const pv_varresampler* vr, const float* x, long long ldx, long long n_in, int channels,
                            float* y, long long ldy, long long n_out, hipStream_t s);

}  // namespace pvhost
#pragma GCC visibility pop
