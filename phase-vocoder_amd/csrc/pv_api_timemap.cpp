// pv_api_timemap.cpp — the time-map stretch of libpv (pv_timemap_*): the
// host split of the map, the handle's map and scan buffers, and the launch sequence of
// pv_timemap_process (analysis, map_sum, map_carry, synthesis_map, seam).  The map is one for all
// channels (pv_timemap_set) or one per channel (pv_timemap_set_channels).
#include <algorithm>
#include <vector>

#include "pv_host.hpp"

namespace pvhost {

namespace {

// a STANDARD time-stretch handle at scale 1 (out hop = hop), N = 256 .. 2048
pv_status check_handle(const char* fn, const pv_handle* h) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    if (h->mode != PV_MODE_STANDARD)
        return fail(PV_ERR_UNSUPPORTED, std::string(fn) + ": REF_COMPAT handle (the time map is the STANDARD time stretch's)");
    if (h->effect != PV_TIME_SHIFT)
        return fail(PV_ERR_UNSUPPORTED, std::string(fn) + ": PV_PITCH_SHIFT handle (the time map is the STANDARD time stretch's)");
    if (h->hs != h->hop)
        return fail(PV_ERR_UNSUPPORTED, std::string(fn) + ": out_hop != hop (the map replaces the scale: create the handle with scale 1)");
    if (h->L_syn < 128 || h->L_syn > 1024)
        return fail(PV_ERR_UNSUPPORTED, std::string(fn) + ": n_samps must be in [256, 2048]");
    return PV_OK;
}

// the map and the scan's run sums and carries: allocated by the first pv_timemap_set, zeroed
pv_status reserve(pv_handle* h) {
    if (h->d_map) return PV_OK;
    const size_t C = (size_t)std::max(h->cfg.max_channels, 1), T = (size_t)std::max(h->cfg.max_frames, 1);
    const size_t R = (size_t)std::max(h->max_runs, 1);
    DevBuf<pv::MapEntry> map;
    DevBuf<unsigned> sum, carry;
    if (map.alloc_zero(T) != hipSuccess || sum.alloc_zero(C * R * h->bins_pad) != hipSuccess ||
        carry.alloc_zero(C * R * h->bins_pad) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PV_ERR_NOMEM, "pv_timemap_set: the map, run sums and carries");
    }
    h->d_map_sum = std::move(sum);
    h->d_map_carry = std::move(carry);
    h->d_map = std::move(map);
    h->map_rows = 1;
    return PV_OK;
}

// the first per-channel set: max_channels rows of max_frames entries and the channels' counts.
// Allocated before anything of the handle's is touched: on PV_ERR_NOMEM the previous state stays
// (the shared map's entries are not carried over: the caller's set replaces them).
pv_status reserve_rows(pv_handle* h, const std::string& fn) {
    const size_t C = (size_t)std::max(h->cfg.max_channels, 1), T = (size_t)std::max(h->cfg.max_frames, 1);
    if (h->map_rows >= (long long)C && h->d_map_counts) return PV_OK;
    DevBuf<pv::MapEntry> map;
    DevBuf<int> counts;
    if (map.alloc_zero(C * T) != hipSuccess || counts.alloc_zero(C) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PV_ERR_NOMEM, fn + ": the channels' maps (max_channels x max_frames entries)");
    }
    h->d_map = std::move(map);
    h->d_map_counts = std::move(counts);
    h->map_rows = (long long)C;
    return PV_OK;
}

}  // namespace

pv_status timemap_set(const char* fn_, pv_handle* h, const double* pos, int n_out) {
    const std::string fn(fn_);
    pv_status st = check_handle(fn_, h);
    if (st != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    if (!pos && n_out == 0) {  // clear (the calls enqueued before it have read their map)
        h->map_n = 0;
        h->map_imax = 0;
        h->map_channels = h->map_counted = 0;
        return PV_OK;
    }
    if (!pos) return fail(PV_ERR_ARG, fn + ": null positions");
    if (n_out < 1 || n_out > h->cfg.max_frames)
        return fail(PV_ERR_ARG, fn + ": n_out must be in [1, max_frames]");
    std::vector<int> idx(n_out);
    std::vector<float> frac(n_out);
    if (!timemap_split(pos, n_out, idx.data(), frac.data()))
        return fail(PV_ERR_ARG, fn + ": every position must be finite, >= 0 and < 2^30");
    std::vector<pv::MapEntry> map(n_out);
    for (int u = 0; u < n_out; ++u) map[u] = pv::MapEntry{idx[u], frac[u]};
    // ordered like the compute calls: the calls enqueued before this one (on any stream) have
    // read the old map before the new one lands, and the first call's zeroing is complete
    PV_HIP(hipDeviceSynchronize());
    if ((st = reserve(h)) != PV_OK) return st;
    PV_HIP(hipMemcpy(h->d_map, map.data(), sizeof(pv::MapEntry) * (size_t)n_out, hipMemcpyHostToDevice));
    PV_HIP(hipDeviceSynchronize());
    h->map_n = n_out;
    h->map_imax = *std::max_element(idx.begin(), idx.end());
    h->map_channels = h->map_counted = 0;  // the shared map replaces a map per channel
    return PV_OK;
}

pv_status timemap_set_channels(const char* fn_, pv_handle* h, const double* pos, long long ld_pos, const int* counts,
                               int channels, int n_out) {
    const std::string fn(fn_);
    pv_status st = check_handle(fn_, h);
    if (st != PV_OK) return st;
    if (!pos) return fail(PV_ERR_ARG, fn + ": null positions");
    if (channels < 1 || channels > h->cfg.max_channels)
        return fail(PV_ERR_ARG, fn + ": channels must be in [1, max_channels]");
    if (n_out < 1 || n_out > h->cfg.max_frames)
        return fail(PV_ERR_ARG, fn + ": n_out must be in [1, max_frames]");
    if (channels > 1 && ld_pos < n_out) return fail(PV_ERR_ARG, fn + ": ld_pos < n_out");
    const size_t T = (size_t)h->cfg.max_frames;
    // rows of max_frames entries; past a channel's count its last entry repeated (valid rows
    // whatever a kernel reads), zeros ({row 0, fraction 0}) past n_out
    std::vector<pv::MapEntry> map((size_t)channels * T, pv::MapEntry{0, 0.0f});
    std::vector<int> cnt((size_t)channels), imax((size_t)channels), idx((size_t)n_out);
    std::vector<float> frac((size_t)n_out);
    bool counted = false;
    for (int c = 0; c < channels; ++c) {
        const int n_c = counts ? counts[c] : n_out;
        const std::string ch = " (channel " + std::to_string(c) + ")";
        if (n_c < 1 || n_c > n_out) return fail(PV_ERR_ARG, fn + ": every count must be in [1, n_out]" + ch);
        if (!timemap_split(pos + (long long)c * ld_pos, n_c, idx.data(), frac.data()))
            return fail(PV_ERR_ARG, fn + ": every position must be finite, >= 0 and < 2^30" + ch);
        pv::MapEntry* row = map.data() + (size_t)c * T;
        for (int u = 0; u < n_out; ++u) {
            const int v = std::min(u, n_c - 1);
            row[u] = pv::MapEntry{idx[(size_t)v], frac[(size_t)v]};
        }
        cnt[(size_t)c] = n_c;
        imax[(size_t)c] = *std::max_element(idx.begin(), idx.begin() + n_c);
        counted = counted || n_c < n_out;
    }
    DeviceGuard g(h->cfg.device);
    // ordered like pv_timemap_set
    PV_HIP(hipDeviceSynchronize());
    if ((st = reserve(h)) != PV_OK || (st = reserve_rows(h, fn)) != PV_OK) return st;
    PV_HIP(hipMemcpy(h->d_map, map.data(), sizeof(pv::MapEntry) * map.size(), hipMemcpyHostToDevice));
    PV_HIP(hipMemcpy(h->d_map_counts, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice));
    PV_HIP(hipDeviceSynchronize());
    h->map_n = n_out;
    h->map_imax_c = std::move(imax);
    h->map_imax = *std::max_element(h->map_imax_c.begin(), h->map_imax_c.end());
    h->map_channels = channels;
    h->map_counted = counted ? 1 : 0;
    return PV_OK;
}

pv_status timemap_check(const char* fn_, const pv_handle* h, const float* x, int channels, int frames,
                        const float* out, long long ldo) {
    const std::string fn(fn_);
    if (h->map_n < 1) return fail(PV_ERR_ARG, fn + ": no map (pv_timemap_set first)");
    if (h->transient) return fail(PV_ERR_ARG, fn + ": not while the transient phase reset is on (pv_set_transient)");
    if (h->pitch_formant)
        return fail(PV_ERR_ARG, fn + ": not while the envelope warp is on (pv_pitch_set_formant)");
    if (frames < 1) return fail(PV_ERR_ARG, fn + ": frames must be at least 1");
    // every row the kernels read, i_u and (for i_u < frames - 1) i_u + 1, is an analysed one: with
    // a map per channel, of the call's channels and their counted frames
    int imax = h->map_imax;
    if (h->map_channels > 0) {
        if (channels > h->map_channels)
            return fail(PV_ERR_ARG, fn + ": more channels than the map has (pv_timemap_channels)");
        imax = *std::max_element(h->map_imax_c.begin(), h->map_imax_c.begin() + channels);
    }
    if (imax > frames - 1)
        return fail(PV_ERR_ARG, fn + ": the map reads past the last analysed frame (max floor(pos) > frames - 1)");
    if (!x || !out) return fail(PV_ERR_ARG, "null x/out");
    if (channels > 1 && ldo < pv_output_length(h, h->map_n))
        return fail(PV_ERR_ARG, "ldo < pv_output_length(h, pv_timemap_frames(h))");
    return PV_OK;
}

pv_status timemap_launch(const char* fn, pv_handle* h, const float* x, long long ldx, long long n_samples,
                         int channels, int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                         hipStream_t s) {
    pv_status st;
    const int n_out = h->map_n;
    const long long olen = pv_output_length(h, n_out);
    if (!spec && (st = own_spectrum(h, fn, s, &spec, &ld_spec)) != PV_OK) return st;
    // every bin analysed (a time stretch reads them all); no run records: the scan is the map's
    if ((st = do_analysis(h, x, ldx, n_samples, channels, frames, spec, ld_spec, false, s)) != PV_OK) return st;

    pv::MapScanParams m{};
    m.spec = reinterpret_cast<const float2*>(spec);
    m.ld_spec = ld_spec;
    m.spec_stride = h->spec_stride;
    m.aframes = frames;
    m.frames = n_out;
    m.F = h->F;
    m.nruns = nruns_of(h, n_out);  // <= max_runs: n_out <= max_frames
    m.L = h->L_syn;
    m.bins_pad = h->bins_pad;
    m.packed = h->packed;
    m.map = h->d_map;
    m.ld_map = h->map_channels > 0 ? h->cfg.max_frames : 0;
    m.counts = h->map_counted ? h->d_map_counts.p : nullptr;
    m.sum = h->d_map_sum;
    m.carry = h->d_map_carry;
    PV_LAUNCH(h, KMS, s, pv::launch_map_sum(channels, m, s));
    PV_LAUNCH(h, KMC, s, pv::launch_map_carry(channels, m, s));

    pv::SynParams p = syn_params(h, spec, ld_spec, n_out, out, ldo, olen);
    p.carry = reinterpret_cast<const int*>(h->d_map_carry.p);
    p.q = 1;  // no output-phase denominator: the phase is the integer sum itself
    p.q_pow2 = 1;
    p.p_mod = 0;
    p.inv_q = 1.0f;
    pv::set_map_args(&p, pv::MapArgs{h->d_map, frames, m.ld_map, m.counts});
    PV_LAUNCH(h, KSM, s, pv::launch_synthesis_map(h->L_syn, h->phase_lock, channels, p, s));
    return do_seam(h, channels, n_out, nullptr, 0, out, ldo, olen, s);
}

pv_status timemap_handle_check(const char* fn, const pv_handle* h) { return check_handle(fn, h); }

}  // namespace pvhost

using namespace pvhost;

extern "C" {

pv_status pv_timemap_split(const double* pos, int n, int* idx, float* frac) {
    if (!pos || !idx || !frac) return fail(PV_ERR_ARG, "pv_timemap_split: null argument");
    if (n <= 0) return fail(PV_ERR_ARG, "pv_timemap_split: n must be positive");
    if (!timemap_split(pos, n, idx, frac))
        return fail(PV_ERR_ARG, "pv_timemap_split: every position must be finite, >= 0 and < 2^30");
    return PV_OK;
}

pv_status pv_timemap_set(pv_handle* h, const double* pos, int n_out) {
    const pv_status st = timemap_set("pv_timemap_set", h, pos, n_out);
    // the map is the caller's again: a pitch map (pv_pitchmap_set), whose stretch map this replaces
    // or clears, is off
    if (st == PV_OK) h->pmap_n = 0;
    return st;
}

pv_status pv_timemap_set_channels(pv_handle* h, const double* pos, long long ld_pos, const int* counts, int channels,
                                  int n_out) {
    const pv_status st = timemap_set_channels("pv_timemap_set_channels", h, pos, ld_pos, counts, channels, n_out);
    if (st == PV_OK) h->pmap_n = 0;  // (as pv_timemap_set: a pitch map is off)
    return st;
}

int pv_timemap_frames(const pv_handle* h) { return h ? h->map_n : 0; }

int pv_timemap_channels(const pv_handle* h) { return (h && h->map_n > 0) ? h->map_channels : 0; }

pv_status pv_timemap_process(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels,
                             int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                             void* stream) {
    pv_status st = check_handle("pv_timemap_process", h);
    if (st != PV_OK || (st = check_common(h, channels, frames)) != PV_OK) return st;
    if (channels == 0) return PV_OK;
    if ((st = timemap_check("pv_timemap_process", h, x, channels, frames, out, ldo)) != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    return timemap_launch("pv_timemap_process", h, x, ldx, n_samples, channels, frames, spec, ld_spec, out, ldo,
                          (hipStream_t)stream);
}

}  // extern "C"
