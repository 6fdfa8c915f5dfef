// pv_api_batch.cpp — the batch pipeline of libpv: the launch sequences and the
// entry points that run them (analysis, resynthesis, process, stream segments, phase locking,
// formant preservation, the handle's own spectrum rows).
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "pv_host.hpp"

namespace pvhost {

namespace {

// the input rows can be read, and the output rows written, two samples at a time
bool in_aligned(const pv_handle* h, const float* x, long long ldx) {
    return (((uintptr_t)x & 7) == 0) && (ldx % 2 == 0) && (h->hop % 2 == 0);
}
bool out_aligned(const float* out, long long ldo) {
    return ((reinterpret_cast<uintptr_t>(out) & 7) == 0) && ((ldo & 1) == 0);
}

// what k_runsum and k_carry share; the carries and the segment state are the caller's
pv::ScanParams scan_params(const pv_handle* h, const pv_float2* spec, long long ld_spec, int frames) {
    pv::ScanParams sc{};
    sc.spec = reinterpret_cast<const float2*>(spec);
    sc.ld_spec = ld_spec;
    sc.spec_stride = h->spec_stride;
    sc.frames = frames;
    sc.F = h->F;
    sc.nruns = nruns_of(h, frames);
    sc.L = h->L_syn;
    sc.bins_pad = h->bins_pad;
    sc.packed = h->packed;
    sc.ek = h->d_ek;
    sc.runsum = h->d_runsum;
    return sc;
}

}  // namespace

// src_hi < 0: every bin analysed (the spectrum is an output); otherwise the bins above it
// may be left out (pv_process without a spectrum buffer: no output bin reads them)
pv_status do_analysis(pv_handle* h, const float* x, long long ldx, long long n, int C, int frames,
                      pv_float2* spec, long long ld_spec, bool want_runsum, hipStream_t s, int src_hi) {
    if (C == 0 || frames == 0) return PV_OK;
    if (!x || !spec) return fail(PV_ERR_ARG, "null x/spec");
    pv_status st = check_ld_spec(h, frames, ld_spec);
    if (st != PV_OK) return st;
    if (C > 1 && ldx < n) return fail(PV_ERR_ARG, "ldx < n_samples");
    pv::AnaParams p{};
    p.x = x;
    p.ldx = ldx;
    p.n = n;
    p.hop = h->hop;
    p.frames = frames;
    p.F = h->F;
    p.nruns = nruns_of(h, frames);
    p.aligned = in_aligned(h, x, ldx);
    p.win = h->d_win;
    p.tw = h->d_tw_ana;
    p.tws = h->d_tws_ana;
    p.ek = h->d_ek;
    p.ek_lane = ek_lane_of(h->cfg.hop_div, h->bins) ? 1 : 0;
    p.spec = reinterpret_cast<float2*>(spec);
    p.ld_spec = ld_spec;
    p.spec_stride = h->spec_stride;
    p.runsum = want_runsum ? h->d_runsum.p : nullptr;
    p.bins_pad = h->bins_pad;
    p.nan_faithful = h->nan_faithful;
    p.packed = h->packed;
    p.src_hi = (src_hi < 0) ? h->L_ana : std::min(src_hi, h->L_ana);
    if (h->mode == PV_MODE_REF_COMPAT) {
        // the REF_COMPAT analysis has no run records: its runs only set which rows a wave
        // writes in turn, and short runs (fewer rows written concurrently per channel, more
        // channels' rows in address order) stream faster (profiles/r05_ab_compat_F.txt);
        // the synthesis keeps h->F (its seams)
        const int fa = h->env.compat_ana_frames;
        p.F = fa;
        p.nruns = (frames + fa - 1) / fa;
    }
    if (h->mode == PV_MODE_STANDARD)
        PV_LAUNCH(h, KA, s, pv::launch_std_analysis(h->L_ana, C, p, s));
    else
        PV_LAUNCH(h, KCA, s, pv::launch_compat_analysis(h->L_ana, C, p, s));
    return PV_OK;
}

// log envelope rows of `frames` frames per channel (k_envelope)
pv_status do_envelope(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames, int order,
                      float* env, long long ld_env, int env_stride, int env_tail, hipStream_t s) {
    pv::EnvParams e{};
    e.spec = reinterpret_cast<const float2*>(spec);
    e.ld_spec = ld_spec;
    e.spec_stride = h->spec_stride;
    e.frames = frames;
    e.F = h->F;
    e.nruns = nruns_of(h, frames);
    e.packed = h->packed;
    e.order = order;
    e.tw = syn_v3_table(h);
    e.tws = h->d_tws_syn;
    e.env = env;
    e.ld_env = ld_env;
    e.env_stride = env_stride;
    e.env_tail = env_tail;
    PV_LAUNCH(h, KENV, s, pv::launch_envelope(h->L_syn, C, e, s));
    return PV_OK;
}

// what every k_synthesis launch of the handle shares (the carries, a segment's offset and a
// mode's own arguments are the caller's)
pv::SynParams syn_params(const pv_handle* h, const pv_float2* spec, long long ld_spec, int frames, float* out,
                         long long ldo, long long olen) {
    pv::SynParams p{};
    p.spec = reinterpret_cast<const float2*>(spec);
    p.ld_spec = ld_spec;
    p.spec_stride = h->spec_stride;
    p.frames = frames;
    p.F = h->F;
    p.nruns = nruns_of(h, frames);
    p.bins_pad = h->bins_pad;
    p.ek = h->d_ek;
    p.jk_mod = h->d_jk_mod;
    p.src_first = h->d_src_first;
    p.src_cnt = h->d_src_cnt;
    p.pitch = h->pitch;
    p.rho = h->rho;
    p.p_mod = h->p_mod;
    p.q = h->q;
    p.q_pow2 = h->q_pow2;
    p.inv_q = h->inv_q;
    p.tw = syn_v3_table(h);
    p.tws = h->d_tws_syn;
    p.gain = h->d_gain;
    p.rot = (h->mode == PV_MODE_REF_COMPAT) ? h->N / 2 : 0;
    p.hs = h->hs;
    p.out = out;
    p.ldo = ldo;
    p.out_len = olen;
    p.out_aligned = out_aligned(out, ldo);
    p.tails = h->d_tails;
    p.tail_len = h->tail_len;
    p.k_lane = h->k_lane;
    p.packed = h->packed;
    p.src_hi = h->src_hi;
    return p;
}

// k_seam after a synthesis of `frames` frames: the workgroups' tails (and ola_in at 0)
pv_status do_seam(pv_handle* h, int C, int frames, const float* ola_in, long long ld_ola, float* out, long long ldo,
                  long long olen, hipStream_t s) {
    const int nruns = nruns_of(h, frames);
    const int nwg = (nruns + 3) / 4;
    if (nwg <= 1 && ola_in == nullptr) return PV_OK;
    pv::SeamParams sm{};
    sm.out = out;
    sm.ldo = ldo;
    sm.out_len = olen;
    sm.tails = h->d_tails;
    sm.ola_in = ola_in;
    sm.ld_ola = ld_ola;
    sm.nruns = nruns;
    sm.nwg = nwg;
    sm.F = h->F;
    sm.hs = h->hs;
    sm.tail_len = h->tail_len;
    PV_LAUNCH(h, KSEAM, s, pv::launch_seam(C, sm, s));
    return PV_OK;
}

// carry_from: unwrap carries already scanned by another handle of the same analysis
// geometry (the harmoniser's voices share one scan); nullptr = scan here.
// env_from: envelope rows already computed by another handle of the same analysis (the
// harmoniser's voices share voice 0's, as they share its carries); nullptr = computed here.
pv_status do_resynthesis(pv_handle* h, const pv_float2* spec, long long ld_spec, int C, int frames,
                         const float* ola_in, long long ld_ola, float* out, long long ldo, bool have_runsum,
                         hipStream_t s, const int* carry_from, bool force_scan, const SegState* seg,
                         const float* env_from) {
    if (C == 0 || frames == 0) {
        return PV_OK;
    }
    if (!spec || !out) return fail(PV_ERR_ARG, "null spec/out");
    const long long olen = pv_output_length(h, frames);
    if (C > 1 && ldo < olen) return fail(PV_ERR_ARG, "ldo < pv_output_length");
    pv_status st = check_ld_spec(h, frames, ld_spec);
    if (st != PV_OK) return st;
    // q = 1 (e.g. pitch 2.0): the output phase rho (phi + 2 pi M) is independent of the
    // unwrap count M mod 1, so no scan is needed
    const bool need_scan = h->mode == PV_MODE_STANDARD && (h->q > 1 || force_scan);
    if (h->transient) {  // (STANDARD + PV_TIME_SHIFT: pv_set_transient)
        if (seg || carry_from || ola_in)
            return fail(PV_ERR_ARG, "transient phase reset: pv_process and pv_pitch_process only");
        if ((st = transient_ready(h, "pv_process", s)) != PV_OK) return st;
        if ((st = transient_flags(h, spec, ld_spec, C, frames, s)) != PV_OK) return st;
    }
    if (need_scan && carry_from == nullptr) {
        pv::ScanParams sc = scan_params(h, spec, ld_spec, frames);
        sc.carry = h->d_carry;
        sc.carry_in = seg ? seg->carry_in : nullptr;
        sc.phi_in = seg ? seg->phi_in : nullptr;
        if (!have_runsum) PV_LAUNCH(h, KRS, s, pv::launch_runsum(C, sc, s));
        PV_LAUNCH(h, KC, s, pv::launch_carry(C, sc, s));
    }
    pv::SynParams p = syn_params(h, spec, ld_spec, frames, out, ldo, olen);
    p.carry = carry_from ? carry_from : (need_scan ? h->d_carry.p : nullptr);
    p.t_off = seg ? seg->t_off : 0u;
    const int smode = (h->mode == PV_MODE_REF_COMPAT) ? 1 : (h->pitch ? 2 : 0);
    if (h->transient) {
        if ((st = transient_offsets(h, spec, ld_spec, C, frames, p.carry, &p, s)) != PV_OK) return st;
        PV_LAUNCH(h, KSR, s, pv::launch_synthesis_reset(h->L_syn, h->phase_lock, C, p, s));
    } else if (h->formant) {  // (STANDARD + PV_PITCH_SHIFT: pv_set_formant)
        const float* env = env_from ? env_from : h->d_env.p;
        if (!env) return fail(PV_ERR_ARG, "formant preservation is on but the handle has no envelope rows");
        const long long ld_env = (long long)h->cfg.max_frames * h->env_stride;
        if (!env_from) {
            pv_status se = do_envelope(h, spec, ld_spec, C, frames, h->formant, h->d_env, ld_env, h->env_stride,
                                       16, s);
            if (se != PV_OK) return se;
        }
        p.env = env;
        p.ld_env = ld_env;
        p.env_stride = h->env_stride;
        PV_LAUNCH(h, KSF, s, pv::launch_synthesis_formant(h->L_syn, C, p, s));
    } else if (h->pitch_formant) {  // (STANDARD + PV_TIME_SHIFT: pv_pitch_set_formant, locked or not)
        if (!h->d_env || !h->d_warp_idx || !h->d_warp_frac)
            return fail(PV_ERR_ARG, "the envelope warp is on but the handle has no envelope rows or warp map");
        const long long ld_env = (long long)h->cfg.max_frames * h->env_stride;
        pv_status se = do_envelope(h, spec, ld_spec, C, frames, h->pitch_formant, h->d_env, ld_env, h->env_stride,
                                   16, s);
        if (se != PV_OK) return se;
        p.env = h->d_env;
        p.ld_env = ld_env;
        p.env_stride = h->env_stride;
        p.src_first = h->d_warp_idx;  // (a time stretch has no pitch map: the fields carry the warp map)
        p.src_cnt = h->d_warp_frac;
        PV_LAUNCH(h, KSW, s, pv::launch_synthesis_warp(h->L_syn, h->phase_lock, C, p, s));
    } else if (h->phase_lock)  // (STANDARD + PV_TIME_SHIFT: pv_set_phase_lock)
        PV_LAUNCH(h, KSL, s, pv::launch_synthesis_locked(h->L_syn, C, p, s));
    else
        PV_LAUNCH(h, KS, s, pv::launch_synthesis(h->L_syn, smode, C, p, s));
    return do_seam(h, C, frames, ola_in, ld_ola, out, ldo, olen, s);
}

// q = 1 (STANDARD): analysis, processing, resynthesis and every seam in one launch
// (pv_fused.hip); outputs equal to do_analysis + do_resynthesis (bit for bit at equal F)
pv_status do_fused(pv_handle* h, const float* x, long long ldx, long long n, int C, int frames, pv_float2* spec,
                   long long ld_spec, float* out, long long ldo, hipStream_t s) {
    if (C == 0 || frames == 0) return PV_OK;
    if (!x || !out) return fail(PV_ERR_ARG, "null x/out");
    // spec == NULL: no spectrum output (the single launch keeps the rows on chip)
    pv_status st = spec ? check_ld_spec(h, frames, ld_spec) : PV_OK;
    if (st != PV_OK) return st;
    if (C > 1 && ldx < n) return fail(PV_ERR_ARG, "ldx < n_samples");
    const long long olen = pv_output_length(h, frames);
    if (C > 1 && ldo < olen) return fail(PV_ERR_ARG, "ldo < pv_output_length");
    const int F = h->F_fused;
    pv::FusedParams p{};
    p.x = x;
    p.ldx = ldx;
    p.n = n;
    p.hop = h->hop;
    p.frames = frames;
    p.F = F;
    p.nruns = (frames + F - 1) / F;
    p.aligned = in_aligned(h, x, ldx);
    p.win = h->d_win;
    p.tw = h->d_tw_syn;    // the stage-major L-point table serves both directions
    p.tws = h->d_tws_syn;  // e^{-2 pi i k/N}, k <= N/2: the analysis split's table too
    p.src_first = h->d_src_first;
    p.src_cnt = h->d_src_cnt;
    p.rho = h->rho;
    p.gain = h->d_gain;
    // pitch 2: the periodic half-size resynthesis (k_fused MODE 4); PV_FUSED_HALF=0 keeps the
    // MODE 3 gather and the full-size inverse FFT (tests compare the two)
    p.tw_half = (tw_syn_len(h->L_syn) == h->L_syn + h->L_syn / 2) ? h->d_tw_syn + h->L_syn : nullptr;
    if (!h->env.fused_half) p.tw_half = nullptr;
    p.hs = h->hs;
    p.spec = reinterpret_cast<float2*>(spec);
    p.ld_spec = ld_spec;
    p.spec_stride = h->spec_stride;
    p.out = out;
    p.ldo = ldo;
    p.out_len = olen;
    p.out_aligned = out_aligned(out, ldo);
    p.tails = h->d_tails;
    p.tail_len = h->tail_len;
    p.seam_flags = h->d_seam_flags;
    p.packed = h->packed;
    p.src_hi = h->src_hi;
    fused_rounds(frames, F, h->env.fused_balance != 0, &p.nwg, &p.n4);  // balanced rounds of the 256 CUs
#ifdef PV_FUSED_STAMPS
    p.stamps = h->d_stamps;
#endif
    PV_LAUNCH(h, KF, s, pv::launch_fused(h->L_syn, h->pitch ? 2 : 0, C, p, s));
    return PV_OK;
}

// One workgroup per channel walks it from its first frame to its last (pv_resident.hip): the
// rows stay in LDS, the decisions are made inline, the handle's F sets the seams.  The caller
// has checked the handle (resident_min) and the alignment of x and out.
pv_status do_resident(pv_handle* h, const float* x, long long ldx, long long n, int C, int frames, float* out,
                      long long ldo, hipStream_t s) {
    if (C == 0 || frames == 0) return PV_OK;
    if (!x || !out) return fail(PV_ERR_ARG, "null x/out");
    if (C > 1 && ldx < n) return fail(PV_ERR_ARG, "ldx < n_samples");
    const long long olen = pv_output_length(h, frames);
    if (C > 1 && ldo < olen) return fail(PV_ERR_ARG, "ldo < pv_output_length");
    pv::ResidentParams p{};
    p.x = x;
    p.ldx = ldx;
    p.n = n;
    p.hop = h->hop;
    p.frames = frames;
    p.F = h->F;
    p.win = h->d_win;
    p.tw = h->d_tw_syn;    // the stage-major L-point table serves both directions
    p.tws = h->d_tws_syn;  // e^{-2 pi i k/N}, k <= N/2: the analysis split's table too
    p.ek = h->d_ek;
    p.jk_mod = h->d_jk_mod;
    p.rho = h->rho;
    p.inv_q = h->inv_q;
    p.p_mod = (unsigned)h->p_mod;
    p.q = (unsigned)h->q;
    p.gain = h->d_gain;
    p.hs = h->hs;
    p.out = out;
    p.ldo = ldo;
    p.out_len = olen;
    PV_LAUNCH(h, KRD, s, pv::launch_resident(h->L_syn, C, p, s));
    return PV_OK;
}

namespace {
// the handle's own spectrum rows (split path, pv_process with spec = NULL): allocated and
// zeroed once, under the handle's lock, so two threads' first calls allocate one buffer
pv_status reserve_spec_own(pv_handle* h) {
    std::lock_guard<std::mutex> lk(h->spec_mu);
    if (h->d_spec_own) return PV_OK;
    const size_t n = (size_t)h->cfg.max_channels * (size_t)h->cfg.max_frames * (size_t)h->spec_stride;
    DevBuf<pv_float2> rows;
    if (rows.alloc(n) != hipSuccess) return fail(PV_ERR_NOMEM, "spectrum rows of a spec = NULL call");
    // (synchronised: the caller's stream may be a non-blocking one, which the null stream's
    // memset would not order before the first analysis)
    if (hipMemset(rows.p, 0, sizeof(pv_float2) * n) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(PV_ERR_HIP, "zeroing the spectrum rows of a spec = NULL call");
    h->d_spec_own = std::move(rows);
    return PV_OK;
}
}  // namespace

// a spec = NULL call on the split path: the handle's own rows, allocated now unless s is being
// captured (an allocation cannot be captured: the rows must exist already then)
pv_status own_spectrum(pv_handle* h, const char* fn, hipStream_t s, pv_float2** spec, long long* ld_spec) {
    bool have;
    {
        std::lock_guard<std::mutex> lk(h->spec_mu);
        have = h->d_spec_own.p != nullptr;
    }
    if (!have) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(PV_ERR_ARG, std::string(fn) + "(spec = NULL) under stream capture: call pv_reserve_spectrum first");
        pv_status st = reserve_spec_own(h);
        if (st != PV_OK) return st;
    }
    *spec = h->d_spec_own;
    *ld_spec = (long long)h->cfg.max_frames * h->spec_stride;
    return PV_OK;
}

namespace {
// the handle's envelope rows (pv_set_formant, pv_pitch_set_formant): allocated once, zeroed
pv_status reserve_env_rows(pv_handle* h, const char* fn) {
    h->env_stride = h->L_syn + 16;
    if (h->d_env) return PV_OK;
    DeviceGuard g(h->cfg.device);
    // rows of N/2 + 16 floats: bin N/2 and 15 zeros make every row store whole 64-byte segments
    const int stride = h->L_syn + 16;
    const size_t n = (size_t)std::max(h->cfg.max_channels, 1) * (size_t)std::max(h->cfg.max_frames, 1) *
                     (size_t)stride;
    DevBuf<float> rows;
    if (rows.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PV_ERR_NOMEM, std::string(fn) + ": envelope rows");
    }
    if (hipMemset(rows.p, 0, sizeof(float) * n) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(PV_ERR_HIP, std::string(fn) + ": zeroing the envelope rows");
    h->d_env = std::move(rows);
    return PV_OK;
}
}  // namespace

pv_status set_formant(pv_handle* h, int order, bool own_rows) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    if (order > 0 && h->transient)
        return fail(PV_ERR_ARG, "pv_set_formant: not while the transient phase reset is on (pv_set_transient)");
    if (h->mode != PV_MODE_STANDARD || h->effect != PV_PITCH_SHIFT)
        return fail(PV_ERR_UNSUPPORTED, "pv_set_formant: STANDARD pitch-shift handles only");
    if (order < 0 || order > h->N / 4) return fail(PV_ERR_ARG, "pv_set_formant: order must be in [0, N/4]");
    if (order > 0 && own_rows) {
        pv_status st = reserve_env_rows(h, "pv_set_formant");
        if (st != PV_OK) return st;
    }
    h->env_stride = h->L_syn + 16;
    h->formant = order;
    return PV_OK;
}

pv_status process_impl(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels, int frames,
                       pv_float2* spec, long long ld_spec, float* out, long long ldo, hipStream_t s) {
    pv_status st = PV_OK;
    if (single_launch(h)) return do_fused(h, x, ldx, n_samples, channels, frames, spec, ld_spec, out, ldo, s);
    // no spectrum output, a plain stretch the resident kernel serves, enough channels to fill the
    // chip with one workgroup each, rows it can read and write two samples at a time: the rows
    // stay on chip (no own-rows buffer: nothing is allocated)
    // (the automatic choice stops at one round of the chip, kResidentRoundChannels: a second,
    // partly filled round runs at one workgroup's latency)
    const bool res_count = channels >= h->resident_min &&
                           (h->env.resident == 1 || channels <= kResidentRoundChannels);
    if (!spec && h->resident_min > 0 && res_count && !h->phase_lock && !h->formant &&
        !h->pitch_formant && !h->transient && in_aligned(h, x, ldx) && out_aligned(out, ldo))
        return do_resident(h, x, ldx, n_samples, channels, frames, out, ldo, s);
    // spec == NULL: the rows go through the handle's own buffer, and bins no output bin reads
    // (pitch > 1) are not analysed
    int src_hi = -1;
    if (!spec && channels > 0 && frames > 0) {
        if ((st = own_spectrum(h, "pv_process", s, &spec, &ld_spec)) != PV_OK) return st;
        // (formant preservation: the envelope at the target bins reads every magnitude)
        if (h->mode == PV_MODE_STANDARD && !h->formant) src_hi = h->src_hi;
    }
    const bool std_mode = (h->mode == PV_MODE_STANDARD) && h->q > 1;  // run records feed the scan
    st = do_analysis(h, x, ldx, n_samples, channels, frames, spec, ld_spec, std_mode, s, src_hi);
    if (st != PV_OK) return st;
    // (single-source pitch: the synthesis reads only the row slots of bins <= src_hi, the
    // ones the analysis wrote, k_synthesis NR)
    return do_resynthesis(h, spec, ld_spec, channels, frames, nullptr, 0, out, ldo, std_mode, s);
}

}  // namespace pvhost

using namespace pvhost;

extern "C" {

pv_status pv_analysis(pv_handle* h, const float* x, long long ldx, long long n_samples,
                      int channels, int frames, pv_float2* spec, long long ld_spec, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    return do_analysis(h, x, ldx, n_samples, channels, frames, spec, ld_spec, false,
                       (hipStream_t)stream);
}

pv_status pv_resynthesis(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                         int frames, const float* ola_in, long long ld_ola, float* out,
                         long long ldo, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (h->transient) return fail(PV_ERR_ARG, "pv_resynthesis: not while the transient phase reset is on (pv_set_transient)");
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    return do_resynthesis(h, spec, ld_spec, channels, frames, ola_in, ld_ola, out, ldo, false,
                          (hipStream_t)stream);
}

int pv_segment_summary_words(const pv_handle* h) {
    return h ? pv::kSegFields * h->bins_pad : 0;
}

// run records of a spectrum (k_runsum, as pv_resynthesis makes them) -> the segment summary
pv_status pv_segment_summary(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                             int frames, int* summary, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (h->mode != PV_MODE_STANDARD) return fail(PV_ERR_UNSUPPORTED, "pv_segment_summary: STANDARD handles only");
    if (h->transient) return fail(PV_ERR_ARG, "pv_segment_summary: not while the transient phase reset is on (pv_set_transient)");
    if (channels == 0) return PV_OK;
    if (!summary) return fail(PV_ERR_ARG, "null summary");
    // (an empty segment has no first or last phase: the caller leaves it out of the order)
    if (frames == 0) return fail(PV_ERR_ARG, "pv_segment_summary: empty segment");
    if (!spec) return fail(PV_ERR_ARG, "null spec");
    if ((st = check_ld_spec(h, frames, ld_spec)) != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    hipStream_t s = (hipStream_t)stream;
    const pv::ScanParams sc = scan_params(h, spec, ld_spec, frames);
    PV_LAUNCH(h, KRS, s, pv::launch_runsum(channels, sc, s));
    pv::SegParams sp{};
    sp.runsum = h->d_runsum;
    sp.nruns = sc.nruns;
    sp.L = h->L_syn;
    sp.bins_pad = h->bins_pad;
    sp.channels = channels;
    sp.ek = h->d_ek;
    sp.summary = summary;
    PV_LAUNCH(h, KRS, s, pv::launch_segsum(sp, s));
    return PV_OK;
}

pv_status pv_segment_resynthesis(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                                 int frames, long long frame0, const int* summaries, int seg, float* out,
                                 long long ldo, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (frame0 < 0 || seg < 0) return fail(PV_ERR_ARG, "negative frame0 / seg");
    if (h->transient)
        return fail(PV_ERR_ARG, "pv_segment_resynthesis: not while the transient phase reset is on (pv_set_transient)");
    if (seg > 0 && !summaries) return fail(PV_ERR_ARG, "null summaries");
    if (channels == 0 || frames == 0) return PV_OK;
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    hipStream_t s = (hipStream_t)stream;
    if (h->mode != PV_MODE_STANDARD)  // no unwrap state: the segment is a plain resynthesis
        return do_resynthesis(h, spec, ld_spec, channels, frames, nullptr, 0, out, ldo, false, s);
    pv::SegParams sp{};
    sp.L = h->L_syn;
    sp.bins_pad = h->bins_pad;
    sp.channels = channels;
    sp.ek = h->d_ek;
    sp.summaries = summaries;
    sp.seg = seg;
    sp.carry_in = h->d_seg_carry;
    sp.phi_in = h->d_seg_phi;
    PV_LAUNCH(h, KC, s, pv::launch_segcarry(sp, s));
    const SegState ss{h->d_seg_carry, h->d_seg_phi, (unsigned)((unsigned long long)frame0 % h->q)};
    return do_resynthesis(h, spec, ld_spec, channels, frames, nullptr, 0, out, ldo, false, s, nullptr,
                          /*force_scan*/ false, &ss);
}

pv_status pv_reserve_spectrum(pv_handle* h) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    DeviceGuard g(h->cfg.device);
    // the single launch keeps a spec = NULL spectrum on chip (with phase locking on, the
    // handle's calls take the split path; with formant preservation on too)
    if (single_launch(h)) return PV_OK;
    return reserve_spec_own(h);
}

pv_status pv_set_phase_lock(pv_handle* h, int lock) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    if (lock != 0 && lock != 1) return fail(PV_ERR_ARG, "pv_set_phase_lock: lock must be 0 or 1");
    pv_status st = check_std_stretch("pv_set_phase_lock", h);
    if (st != PV_OK) return st;
    h->phase_lock = lock;
    return PV_OK;
}

int pv_get_phase_lock(const pv_handle* h) { return h ? h->phase_lock : 0; }

pv_status pv_set_formant(pv_handle* h, int order) { return set_formant(h, order, true); }

int pv_get_formant(const pv_handle* h) { return h ? h->formant : 0; }

pv_status pv_pitch_set_formant(pv_handle* h, int order) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    pv_status st = check_std_stretch("pv_pitch_set_formant", h);
    if (st != PV_OK) return st;
    if (order < 0 || order > h->N / 4) return fail(PV_ERR_ARG, "pv_pitch_set_formant: order must be in [0, N/4]");
    if (order > 0 && h->transient)
        return fail(PV_ERR_ARG, "pv_pitch_set_formant: not while the transient phase reset is on (pv_set_transient)");
    if (order > 0) {
        // on a failure the feature stays as it was (off, on a first call)
        if ((st = reserve_env_rows(h, "pv_pitch_set_formant")) != PV_OK) return st;
        // (the map is the handle's own, hop and out hop only: not part of the table blob, so a
        // tables_external handle builds it here like any other)
        if (!h->d_warp_idx || !h->d_warp_frac) {
            DeviceGuard g(h->cfg.device);
            std::vector<int> idx, bits;
            std::vector<float> frac;
            warp_map(h->bins, h->hop, h->hs, idx, frac);
            bits.resize(frac.size());
            std::memcpy(bits.data(), frac.data(), sizeof(float) * frac.size());
            DevBuf<int> di, df;
            if (di.upload(idx.data(), idx.size()) != hipSuccess || df.upload(bits.data(), bits.size()) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PV_ERR_NOMEM, "pv_pitch_set_formant: warp map");
            }
            h->d_warp_idx = std::move(di);
            h->d_warp_frac = std::move(df);
        }
    }
    h->pitch_formant = order;
    return PV_OK;
}

int pv_pitch_get_formant(const pv_handle* h) { return h ? h->pitch_formant : 0; }

pv_status pv_spectral_envelope(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels, int frames,
                               int order, float* env, long long ld_env, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (h->mode != PV_MODE_STANDARD) return fail(PV_ERR_UNSUPPORTED, "pv_spectral_envelope: STANDARD handles only");
    if (order < 1 || order > h->N / 4) return fail(PV_ERR_ARG, "pv_spectral_envelope: order must be in [1, N/4]");
    if (channels == 0 || frames == 0) return PV_OK;
    if (!spec || !env) return fail(PV_ERR_ARG, "null spec/env");
    if ((st = check_ld_spec(h, frames, ld_spec)) != PV_OK) return st;
    // rows of N/2 + 8 floats, the natural layout's spec_stride (a packed handle's N/2 slots
    // cannot hold the N/2 + 1 values)
    const int stride = h->L_syn + 8;
    if (ld_env < (long long)frames * stride) return fail(PV_ERR_ARG, "ld_env < frames * (N/2 + 8)");
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    return do_envelope(h, spec, ld_spec, channels, frames, order, env, ld_env, stride, 1, (hipStream_t)stream);
}

pv_status pv_process(pv_handle* h, const float* x, long long ldx, long long n_samples,
                     int channels, int frames, pv_float2* spec, long long ld_spec, float* out,
                     long long ldo, void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    return process_impl(h, x, ldx, n_samples, channels, frames, spec, ld_spec, out, ldo, (hipStream_t)stream);
}

}  // extern "C"
