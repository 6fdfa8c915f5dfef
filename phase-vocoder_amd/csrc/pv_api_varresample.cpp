// pv_api_varresample.cpp — the variable-rate resampler of libpv and the pitch map built on it
// (DESIGN.md §3.13).  pv_varresampler (pv_host.hpp): a quality preset, a block length and the
// device records of the current map, {T_b, d_b, Sq_b, W_b} per block and the staged input span
// per tile (pv_varresample.hpp), both built on the host by pv_varresampler_set_map;
// pv_varresampler_set_maps: the same per channel;
// pv_pitchmap_*: the plan (pv_tables.cpp), the stretch map installed as pv_timemap_set installs
// one, and pv_timemap_process into the handle's scratch rows followed by pv_varresample.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pv_host.hpp"

namespace pvhost {

namespace {

// tiles of kVarTile outputs that max_blocks blocks make: the row length of the tile records
size_t var_tiles_cap(const pv_varresampler* vr) {
    return (size_t)(((long long)vr->max_blocks * vr->block + pv::kVarTile - 1) / pv::kVarTile);
}

// One map's validation and records (pv_varresampler_set_map, and pv_varresampler_set_maps per
// channel): copy (every step 2^32, no fraction in the start: the rows shifted by `shift`, no
// records), or the per-block records {T, d, Sq, W} and the per-tile input spans.
struct VarRecords {
    bool copy = false;
    long long shift = 0;
    std::vector<pv::VarBlock> blocks;
    std::vector<pv::VarTile> tiles;
    int span4_max = 0;
};
pv_status var_records(const std::string& fn, const std::string& who, const pv_varresampler* vr, long long start,
                      const long long* step, int nblocks, VarRecords* out) {
    if (start < 0) return fail(PV_ERR_ARG, fn + ": negative start" + who);
    const int B = vr->block;
    bool ones = (start & 0xffffffffLL) == 0;
    long long T = start;
    for (int b = 0; b < nblocks; ++b) {
        if (step[b] < kVarStepMin || step[b] > kVarStepMax)
            return fail(PV_ERR_ARG, fn + ": every step must be in [2^30, 2^34] (ratio 1/4 .. 4)" + who);
        ones = ones && step[b] == kVarOne;
        if (T > (1LL << 62) - (long long)B * step[b]) return fail(PV_ERR_ARG, fn + ": the positions leave 62 bits" + who);
        T += (long long)B * step[b];
    }
    if (ones) {
        out->copy = true;
        out->shift = start >> 32;
        return PV_OK;
    }
    const long long length = (long long)nblocks * B;
    const int ntiles = (int)((length + pv::kVarTile - 1) / pv::kVarTile);
    out->blocks.assign((size_t)nblocks, pv::VarBlock{});
    std::vector<long long> lo((size_t)ntiles, INT64_MAX), hi((size_t)ntiles, INT64_MIN);
    T = start;
    for (int b = 0; b < nblocks; ++b) {
        pv::VarBlock& r = out->blocks[(size_t)b];
        r.T = T;
        r.d = step[b];
        var_block_filter(r.d, vr->quality, &r.Sq, &r.W);
        // the input samples this block's outputs read, tile by tile: i - W + 1 .. i + W
        const long long m0 = (long long)b * B, m1 = m0 + B - 1;
        for (long long t = m0 / pv::kVarTile; t <= m1 / pv::kVarTile; ++t) {
            const long long jlo = std::max(m0, t * pv::kVarTile) - m0;
            const long long jhi = std::min(m1, t * pv::kVarTile + pv::kVarTile - 1) - m0;
            lo[(size_t)t] = std::min(lo[(size_t)t], ((r.T + jlo * r.d) >> 32) - r.W + 1);
            hi[(size_t)t] = std::max(hi[(size_t)t], ((r.T + jhi * r.d) >> 32) + r.W);
        }
        T += (long long)B * r.d;
    }
    out->tiles.assign((size_t)ntiles, pv::VarTile{});
    for (int t = 0; t < ntiles; ++t) {
        // up to 3 samples before `base` for the 16-byte alignment, then whole 16-byte slots
        const long long span4 = (hi[(size_t)t] - lo[(size_t)t] + 1 + 3 + 3) / 4;
        if (span4 * 16 > pv::kResampleLdsBytes)
            return fail(PV_ERR_UNSUPPORTED, fn + ": a tile's input span exceeds the LDS budget" + who);
        out->tiles[(size_t)t] = pv::VarTile{lo[(size_t)t], (int)span4, 0};
        out->span4_max = std::max(out->span4_max, (int)span4);
    }
    return PV_OK;
}

}  // namespace

hipError_t varresample_rows(const pv_varresampler* vr, const float* x, long long ldx, long long n_in, int channels,
                            float* y, long long ldy, long long n_out, hipStream_t s) {
    const bool per_channel = vr->map_channels > 0;
    if (vr->copy)
        return pv::launch_var_copy(x, ldx, n_in, vr->copy_shift, per_channel ? vr->d_shift_c.p : nullptr, y, ldy, n_out,
                                   channels, s);
    pv::VarResampleParams p{};
    p.x = x;
    p.ldx = ldx;
    p.n_in = n_in;
    p.y = y;
    p.ldy = ldy;
    p.n_out = n_out;
    p.blocks = per_channel ? vr->d_blocks_c : vr->d_blocks;
    p.tiles = per_channel ? vr->d_tiles_c : vr->d_tiles;
    p.ld_blocks = per_channel ? vr->max_blocks : 0;
    p.ld_tiles = per_channel ? (long long)var_tiles_cap(vr) : 0;
    p.copy_shift = per_channel ? vr->d_shift_c.p : nullptr;
    p.win = vr->d_win;
    p.B = vr->block;
    p.ntiles = (int)((n_out + pv::kVarTile - 1) / pv::kVarTile);
    p.win_scale = (float)((double)pv::kVarWinN / resample_zero_crossings(vr->quality) * 0x1p-32);
    return pv::launch_var_resample(channels, p, vr->span4_max, s);
}

}  // namespace pvhost

using namespace pvhost;

extern "C" {

pv_status pv_varresample_steps(const double* ratio, int n, long long* step) {
    if (!ratio || !step) return fail(PV_ERR_ARG, "pv_varresample_steps: null argument");
    if (n <= 0) return fail(PV_ERR_ARG, "pv_varresample_steps: n must be positive");
    if (!varresample_steps(ratio, n, step))
        return fail(PV_ERR_ARG, "pv_varresample_steps: every ratio must be finite and in [1/4, 4]");
    return PV_OK;
}

pv_status pv_varresampler_create(int quality, int block, int max_blocks, int device, pv_varresampler** out) {
    if (!out) return fail(PV_ERR_ARG, "null argument");
    *out = nullptr;
    pv_status st = check_quality("pv_varresampler_create", quality);
    if (st != PV_OK) return st;
    if (block < 16 || block > 4096) return fail(PV_ERR_ARG, "pv_varresampler_create: block must be in [16, 4096]");
    if (max_blocks < 1 || (long long)max_blocks * block > 0x7fffffffLL)
        return fail(PV_ERR_ARG, "pv_varresampler_create: max_blocks must be positive, max_blocks * block < 2^31");
    std::unique_ptr<pv_varresampler> vr(new pv_varresampler());
    vr->quality = quality;
    vr->block = block;
    vr->max_blocks = max_blocks;
    vr->device = device;
    std::vector<float> win;
    var_window_table(quality, pv::kVarWinN, pv::kVarWinLen, win);
    const size_t ntiles = var_tiles_cap(vr.get());
    DeviceGuard dg(device);
    if (vr->d_blocks.alloc_zero((size_t)max_blocks) != hipSuccess || vr->d_tiles.alloc_zero(ntiles) != hipSuccess ||
        vr->d_win.upload(reinterpret_cast<const float2*>(win.data()), win.size() / 2) != hipSuccess) {
        (void)hipGetLastError();
        vr->d_blocks.reset();
        vr->d_tiles.reset();
        vr->d_win.reset();
        return fail(PV_ERR_NOMEM, "pv_varresampler_create: the block and tile records and the window table");
    }
    PV_HIP(hipDeviceSynchronize());
    *out = vr.release();
    return PV_OK;
}

void pv_varresampler_destroy(pv_varresampler* vr) {
    if (!vr) return;
    {
        DeviceGuard dg(vr->device);
        vr->d_blocks.reset();
        vr->d_tiles.reset();
        vr->d_win.reset();
        vr->d_blocks_c.reset();
        vr->d_tiles_c.reset();
        vr->d_shift_c.reset();
    }
    delete vr;
}

pv_status pv_varresampler_set_map(pv_varresampler* vr, long long start, const long long* step, int nblocks) {
    if (!vr) return fail(PV_ERR_ARG, "null variable-rate resampler");
    if (!step) return fail(PV_ERR_ARG, "pv_varresampler_set_map: null steps");
    if (nblocks < 1 || nblocks > vr->max_blocks)
        return fail(PV_ERR_ARG, "pv_varresampler_set_map: nblocks must be in [1, max_blocks]");
    VarRecords r;
    const pv_status st = var_records("pv_varresampler_set_map", "", vr, start, step, nblocks, &r);
    if (st != PV_OK) return st;
    DeviceGuard dg(vr->device);
    if (r.copy) {  // ratio 1 throughout: the shifted copy, no filter, no records
        PV_HIP(hipDeviceSynchronize());
        vr->copy = 1;
        vr->copy_shift = r.shift;
        vr->nblocks = nblocks;
        vr->map_channels = 0;
        return PV_OK;
    }
    // ordered like the compute calls: the calls enqueued before this one (on any stream) have
    // read the old records before the new ones land
    PV_HIP(hipDeviceSynchronize());
    PV_HIP(hipMemcpy(vr->d_blocks, r.blocks.data(), sizeof(pv::VarBlock) * r.blocks.size(), hipMemcpyHostToDevice));
    PV_HIP(hipMemcpy(vr->d_tiles, r.tiles.data(), sizeof(pv::VarTile) * r.tiles.size(), hipMemcpyHostToDevice));
    PV_HIP(hipDeviceSynchronize());
    vr->copy = 0;
    vr->copy_shift = 0;
    vr->span4_max = r.span4_max;
    vr->nblocks = nblocks;
    vr->map_channels = 0;  // the shared map replaces maps per channel
    return PV_OK;
}

pv_status pv_varresampler_set_maps(pv_varresampler* vr, int channels, const long long* start, const long long* step,
                                   long long ld_step, int nblocks) {
    const char* fn = "pv_varresampler_set_maps";
    if (!vr) return fail(PV_ERR_ARG, "null variable-rate resampler");
    if (!start || !step) return fail(PV_ERR_ARG, std::string(fn) + ": null starts / steps");
    if (channels < 1) return fail(PV_ERR_ARG, std::string(fn) + ": channels must be positive");
    if (nblocks < 1 || nblocks > vr->max_blocks)
        return fail(PV_ERR_ARG, std::string(fn) + ": nblocks must be in [1, max_blocks]");
    if (channels > 1 && ld_step < nblocks) return fail(PV_ERR_ARG, std::string(fn) + ": ld_step < nblocks");
    const size_t ldb = (size_t)vr->max_blocks, ldt = var_tiles_cap(vr);
    // a copy channel's records stay zero (its workgroups never read them)
    std::vector<pv::VarBlock> blocks((size_t)channels * ldb, pv::VarBlock{0, 0, 0u, 0});
    std::vector<pv::VarTile> tiles((size_t)channels * ldt, pv::VarTile{0, 0, 0});
    std::vector<long long> shift((size_t)channels);
    int span4_max = 0;
    bool all_copy = true;
    for (int c = 0; c < channels; ++c) {
        VarRecords r;
        const pv_status st = var_records(fn, " (channel " + std::to_string(c) + ")", vr, start[c],
                                         step + (long long)c * ld_step, nblocks, &r);
        if (st != PV_OK) return st;
        shift[(size_t)c] = r.copy ? r.shift : -1;
        all_copy = all_copy && r.copy;
        if (r.copy) continue;
        std::copy(r.blocks.begin(), r.blocks.end(), blocks.begin() + (size_t)c * ldb);
        std::copy(r.tiles.begin(), r.tiles.end(), tiles.begin() + (size_t)c * ldt);
        span4_max = std::max(span4_max, r.span4_max);
    }
    DeviceGuard dg(vr->device);
    PV_HIP(hipDeviceSynchronize());
    if (channels > vr->cap_channels) {  // allocated before the old records go: on PV_ERR_NOMEM they stay
        DevBuf<pv::VarBlock> nb;
        DevBuf<pv::VarTile> nt;
        DevBuf<long long> ns;
        if (nb.alloc_zero((size_t)channels * ldb) != hipSuccess || nt.alloc_zero((size_t)channels * ldt) != hipSuccess ||
            ns.alloc_zero((size_t)channels) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PV_ERR_NOMEM, std::string(fn) + ": the channels' block and tile records");
        }
        vr->d_blocks_c = std::move(nb);
        vr->d_tiles_c = std::move(nt);
        vr->d_shift_c = std::move(ns);
        vr->cap_channels = channels;
    }
    PV_HIP(hipMemcpy(vr->d_blocks_c, blocks.data(), sizeof(pv::VarBlock) * blocks.size(), hipMemcpyHostToDevice));
    PV_HIP(hipMemcpy(vr->d_tiles_c, tiles.data(), sizeof(pv::VarTile) * tiles.size(), hipMemcpyHostToDevice));
    PV_HIP(hipMemcpy(vr->d_shift_c, shift.data(), sizeof(long long) * shift.size(), hipMemcpyHostToDevice));
    PV_HIP(hipDeviceSynchronize());
    vr->copy = all_copy ? 1 : 0;
    vr->copy_shift = 0;
    vr->span4_max = span4_max;
    vr->nblocks = nblocks;
    vr->map_channels = channels;
    return PV_OK;
}

int pv_varresample_map_channels(const pv_varresampler* vr) { return (vr && vr->nblocks > 0) ? vr->map_channels : 0; }

long long pv_varresample_length(const pv_varresampler* vr) { return vr ? (long long)vr->nblocks * vr->block : 0; }

pv_status pv_varresample(pv_varresampler* vr, const float* x, long long ldx, long long n_in, int channels, float* y,
                         long long ldy, long long n_out, void* stream) {
    if (!vr) return fail(PV_ERR_ARG, "null variable-rate resampler");
    if (channels < 0 || n_in < 0 || n_out < 0) return fail(PV_ERR_ARG, "negative channels / n_in / n_out");
    if (vr->nblocks < 1) return fail(PV_ERR_ARG, "pv_varresample: no map (pv_varresampler_set_map first)");
    if (n_out > pv_varresample_length(vr)) return fail(PV_ERR_ARG, "pv_varresample: n_out > pv_varresample_length");
    if (vr->map_channels > 0 && channels > vr->map_channels)
        return fail(PV_ERR_ARG, "pv_varresample: more channels than the maps (pv_varresample_map_channels)");
    if (channels == 0 || n_out == 0) return PV_OK;
    if (!x || !y) return fail(PV_ERR_ARG, "null x/y");
    if (channels > 1 && (ldx < n_in || ldy < n_out)) return fail(PV_ERR_ARG, "ldx < n_in or ldy < n_out");
    const float* xe = x + (channels - 1) * ldx + n_in;
    const float* ye = y + (channels - 1) * ldy + n_out;
    if ((uintptr_t)x < (uintptr_t)ye && (uintptr_t)y < (uintptr_t)xe) return fail(PV_ERR_ARG, "x and y overlap");
    DeviceGuard dg(vr->device);
    const hipError_t e = varresample_rows(vr, x, ldx, n_in, channels, y, ldy, n_out, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("var_resample launch: ") + hipGetErrorString(e));
    return PV_OK;
}

// ------------------------------------------------------------------ the pitch map
pv_status pv_pitchmap_plan(int n_samps, int hop, const double* pos, const double* ratio, int n, double* pos_s,
                           int cap_s, int* n_s, long long* step, int cap_steps, int* n_steps) {
    if (!pos || !ratio || !pos_s || !n_s || !step || !n_steps) return fail(PV_ERR_ARG, "pv_pitchmap_plan: null argument");
    std::vector<double> ps;
    std::vector<long long> st;
    if (!pitchmap_plan(n_samps, hop, pos, ratio, n, ps, st))
        return fail(PV_ERR_ARG, "pv_pitchmap_plan: n >= 1, n * hop < 2^28, 1 <= hop <= n_samps, every position finite, "
                                ">= 0 and < 2^30, every ratio finite and in [1/4, 4]");
    if ((long long)ps.size() > cap_s || (long long)st.size() > cap_steps)
        return fail(PV_ERR_ARG, "pv_pitchmap_plan: pos_s or step too small (up to 4 n + 1 positions, "
                                "ceil((n hop + n_samps - hop) / hop) steps)");
    std::copy(ps.begin(), ps.end(), pos_s);
    std::copy(st.begin(), st.end(), step);
    *n_s = (int)ps.size();
    *n_steps = (int)st.size();
    return PV_OK;
}

namespace {

// the scratch rows of the stretch and the handle's variable-rate resampler at `quality` (the
// caller holds the device guard)
pv_status pitchmap_reserve(const char* fn, pv_handle* h, int quality) {
    const long long rows = pv_output_length(h, std::max(h->cfg.max_frames, 1));
    // (rows of a multiple of 4 floats, shared with pv_pitch_reserve: whichever comes first allocates)
    if (!h->d_pitch) {
        const long long ld = (rows + 3) & ~3LL;
        if (h->d_pitch.alloc((size_t)ld * (size_t)std::max(h->cfg.max_channels, 1)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PV_ERR_NOMEM, std::string(fn) + ": scratch rows");
        }
        h->ld_pitch = ld;
    }
    if (h->pmap_vr && h->pmap_vr->quality != quality) {
        (void)hipDeviceSynchronize();  // calls in flight read the old records
        pv_varresampler_destroy(h->pmap_vr);
        h->pmap_vr = nullptr;
        h->pmap_n = 0;
    }
    if (!h->pmap_vr) {
        const long long max_blocks = (rows + h->hop - 1) / h->hop;
        return pv_varresampler_create(quality, h->hop, (int)max_blocks, h->cfg.device, &h->pmap_vr);
    }
    return PV_OK;
}

}  // namespace

pv_status pv_pitchmap_set(pv_handle* h, const double* pos, const double* ratio, int n, int quality) {
    pv_status st = timemap_handle_check("pv_pitchmap_set", h);
    if (st != PV_OK) return st;
    if (!pos && !ratio && n == 0) {  // clear: the stretch map goes with it
        if (h->pmap_n > 0) st = timemap_set("pv_pitchmap_set", h, nullptr, 0);
        h->pmap_n = 0;
        return st;
    }
    if (!pos || !ratio) return fail(PV_ERR_ARG, "pv_pitchmap_set: null positions / ratios");
    if ((st = check_quality("pv_pitchmap_set", quality)) != PV_OK) return st;
    if (n < 1 || n > h->cfg.max_frames) return fail(PV_ERR_ARG, "pv_pitchmap_set: n must be in [1, max_frames]");
    if (h->hop < 16 || h->hop > 4096) return fail(PV_ERR_UNSUPPORTED, "pv_pitchmap_set: the hop must be in [16, 4096]");
    std::vector<double> pos_s;
    std::vector<long long> step;
    if (!pitchmap_plan(h->N, h->hop, pos, ratio, n, pos_s, step))
        return fail(PV_ERR_ARG, "pv_pitchmap_set: n * hop < 2^28, every position finite, >= 0 and < 2^30, every "
                                "ratio finite and in [1/4, 4]");
    if ((long long)pos_s.size() > h->cfg.max_frames)
        return fail(PV_ERR_ARG, "pv_pitchmap_set: the stretch needs more than max_frames frames (sum of the ratios)");
    DeviceGuard g(h->cfg.device);
    if ((st = pitchmap_reserve("pv_pitchmap_set", h, quality)) != PV_OK) return st;
    st = pv_varresampler_set_map(h->pmap_vr, 0, step.data(), (int)step.size());
    if (st == PV_OK) st = timemap_set("pv_pitchmap_set", h, pos_s.data(), (int)pos_s.size());
    // (a failure here is the device's: the two halves may no longer belong together)
    h->pmap_n = st == PV_OK ? n : 0;
    return st;
}

pv_status pv_pitchmap_set_channels(pv_handle* h, const double* pos, long long ld_pos, const double* ratio,
                                   long long ld_ratio, int channels, int n, int quality) {
    const char* fn = "pv_pitchmap_set_channels";
    const std::string f(fn);
    pv_status st = timemap_handle_check(fn, h);
    if (st != PV_OK) return st;
    if (!pos || !ratio) return fail(PV_ERR_ARG, f + ": null positions / ratios");
    if ((st = check_quality(fn, quality)) != PV_OK) return st;
    if (channels < 1 || channels > h->cfg.max_channels)
        return fail(PV_ERR_ARG, f + ": channels must be in [1, max_channels]");
    if (n < 1 || n > h->cfg.max_frames) return fail(PV_ERR_ARG, f + ": n must be in [1, max_frames]");
    if (channels > 1 && (ld_pos < n || ld_ratio < n)) return fail(PV_ERR_ARG, f + ": ld_pos < n or ld_ratio < n");
    if (h->hop < 16 || h->hop > 4096) return fail(PV_ERR_UNSUPPORTED, f + ": the hop must be in [16, 4096]");
    // the plan per channel: its stretch positions (n_s[c] of them) and its steps (as many for every
    // channel: the blocks of the final output)
    std::vector<std::vector<double>> pos_s((size_t)channels);
    std::vector<long long> steps;
    std::vector<int> n_s((size_t)channels);
    size_t nsteps = 0;
    int n_max = 0;
    for (int c = 0; c < channels; ++c) {
        const std::string ch = " (channel " + std::to_string(c) + ")";
        std::vector<long long> step;
        if (!pitchmap_plan(h->N, h->hop, pos + (long long)c * ld_pos, ratio + (long long)c * ld_ratio, n,
                           pos_s[(size_t)c], step))
            return fail(PV_ERR_ARG, f + ": n * hop < 2^28, every position finite, >= 0 and < 2^30, every ratio "
                                        "finite and in [1/4, 4]" + ch);
        if ((long long)pos_s[(size_t)c].size() > h->cfg.max_frames)
            return fail(PV_ERR_ARG, f + ": the stretch needs more than max_frames frames (sum of the ratios)" + ch);
        if (c == 0) {
            nsteps = step.size();
            steps.resize((size_t)channels * nsteps);
        }
        std::copy(step.begin(), step.end(), steps.begin() + (size_t)c * nsteps);
        n_s[(size_t)c] = (int)pos_s[(size_t)c].size();
        n_max = std::max(n_max, n_s[(size_t)c]);
    }
    // rows of n_max positions, a channel's last repeated past its own n_s
    std::vector<double> rows((size_t)channels * (size_t)n_max);
    for (int c = 0; c < channels; ++c)
        for (int v = 0; v < n_max; ++v)
            rows[(size_t)c * (size_t)n_max + (size_t)v] = pos_s[(size_t)c][(size_t)std::min(v, n_s[(size_t)c] - 1)];
    const std::vector<long long> start((size_t)channels, 0);
    DeviceGuard g(h->cfg.device);
    if ((st = pitchmap_reserve(fn, h, quality)) != PV_OK) return st;
    st = pv_varresampler_set_maps(h->pmap_vr, channels, start.data(), steps.data(), (long long)nsteps, (int)nsteps);
    if (st == PV_OK) st = timemap_set_channels(fn, h, rows.data(), n_max, n_s.data(), channels, n_max);
    // (a failure here is the device's: the two halves may no longer belong together)
    h->pmap_n = st == PV_OK ? n : 0;
    return st;
}

long long pv_pitchmap_output_length(const pv_handle* h) {
    return (h && h->pmap_n > 0) ? pv_output_length(h, h->pmap_n) : 0;
}

pv_status pv_pitchmap_process(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels,
                              int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                              void* stream) {
    pv_status st = timemap_handle_check("pv_pitchmap_process", h);
    if (st != PV_OK || (st = check_common(h, channels, frames)) != PV_OK) return st;
    if (channels == 0) return PV_OK;
    if (h->pmap_n < 1) return fail(PV_ERR_ARG, "pv_pitchmap_process: no pitch map (pv_pitchmap_set first)");
    if ((st = timemap_check("pv_pitchmap_process", h, x, channels, frames, h->d_pitch, h->ld_pitch)) != PV_OK) return st;
    if (!out) return fail(PV_ERR_ARG, "null x/out");
    const long long n_mid = pv_output_length(h, h->map_n), n_fin = pv_output_length(h, h->pmap_n);
    if (channels > 1 && ldo < n_fin) return fail(PV_ERR_ARG, "ldo < pv_pitchmap_output_length");
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    hipStream_t s = (hipStream_t)stream;
    st = timemap_launch("pv_pitchmap_process", h, x, ldx, n_samples, channels, frames, spec, ld_spec, h->d_pitch,
                        h->ld_pitch, s);
    if (st != PV_OK) return st;
    PV_LAUNCH(h, KVR, s, varresample_rows(h->pmap_vr, h->d_pitch, h->ld_pitch, n_mid, channels, out, ldo, n_fin, s));
    return PV_OK;
}

}  // extern "C"
