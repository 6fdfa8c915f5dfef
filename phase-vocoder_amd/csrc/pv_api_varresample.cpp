// pv_api_varresample.cpp — the variable-rate resampler of libpv and the pitch map built on it
// (DESIGN.md §3.13).  pv_varresampler (pv_host.hpp): a quality preset, a block length and the
// device records of the current map, {T_b, d_b, Sq_b, W_b} per block and the staged input span
// per tile (pv_varresample.hpp), both built on the host by pv_varresampler_set_map;
// pv_pitchmap_*: the plan (pv_tables.cpp), the stretch map installed as pv_timemap_set installs
// one, and pv_timemap_process into the handle's scratch rows followed by pv_varresample.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pv_host.hpp"

namespace pvhost {

hipError_t varresample_rows(const pv_varresampler* vr, const float* x, long long ldx, long long n_in, int channels,
                            float* y, long long ldy, long long n_out, hipStream_t s) {
    if (vr->copy) return pv::launch_var_copy(x, ldx, n_in, vr->copy_shift, y, ldy, n_out, channels, s);
    pv::VarResampleParams p{};
    p.x = x;
    p.ldx = ldx;
    p.n_in = n_in;
    p.y = y;
    p.ldy = ldy;
    p.n_out = n_out;
    p.blocks = vr->d_blocks;
    p.tiles = vr->d_tiles;
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
    const size_t ntiles = (size_t)(((long long)max_blocks * block + pv::kVarTile - 1) / pv::kVarTile);
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
    }
    delete vr;
}

pv_status pv_varresampler_set_map(pv_varresampler* vr, long long start, const long long* step, int nblocks) {
    if (!vr) return fail(PV_ERR_ARG, "null variable-rate resampler");
    if (!step) return fail(PV_ERR_ARG, "pv_varresampler_set_map: null steps");
    if (nblocks < 1 || nblocks > vr->max_blocks)
        return fail(PV_ERR_ARG, "pv_varresampler_set_map: nblocks must be in [1, max_blocks]");
    if (start < 0) return fail(PV_ERR_ARG, "pv_varresampler_set_map: negative start");
    const int B = vr->block;
    bool ones = (start & 0xffffffffLL) == 0;
    long long T = start;
    for (int b = 0; b < nblocks; ++b) {
        if (step[b] < kVarStepMin || step[b] > kVarStepMax)
            return fail(PV_ERR_ARG, "pv_varresampler_set_map: every step must be in [2^30, 2^34] (ratio 1/4 .. 4)");
        ones = ones && step[b] == kVarOne;
        if (T > (1LL << 62) - (long long)B * step[b])
            return fail(PV_ERR_ARG, "pv_varresampler_set_map: the positions leave 62 bits");
        T += (long long)B * step[b];
    }
    DeviceGuard dg(vr->device);
    if (ones) {  // ratio 1 throughout: the shifted copy, no filter, no records
        PV_HIP(hipDeviceSynchronize());
        vr->copy = 1;
        vr->copy_shift = start >> 32;
        vr->nblocks = nblocks;
        return PV_OK;
    }
    const long long length = (long long)nblocks * B;
    const int ntiles = (int)((length + pv::kVarTile - 1) / pv::kVarTile);
    std::vector<pv::VarBlock> blocks((size_t)nblocks);
    std::vector<long long> lo((size_t)ntiles, INT64_MAX), hi((size_t)ntiles, INT64_MIN);
    T = start;
    for (int b = 0; b < nblocks; ++b) {
        pv::VarBlock& r = blocks[(size_t)b];
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
    std::vector<pv::VarTile> tiles((size_t)ntiles);
    int span4_max = 0;
    for (int t = 0; t < ntiles; ++t) {
        // up to 3 samples before `base` for the 16-byte alignment, then whole 16-byte slots
        const long long span4 = (hi[(size_t)t] - lo[(size_t)t] + 1 + 3 + 3) / 4;
        if (span4 * 16 > pv::kResampleLdsBytes)
            return fail(PV_ERR_UNSUPPORTED, "pv_varresampler_set_map: a tile's input span exceeds the LDS budget");
        tiles[(size_t)t] = pv::VarTile{lo[(size_t)t], (int)span4, 0};
        span4_max = std::max(span4_max, (int)span4);
    }
    // ordered like the compute calls: the calls enqueued before this one (on any stream) have
    // read the old records before the new ones land
    PV_HIP(hipDeviceSynchronize());
    PV_HIP(hipMemcpy(vr->d_blocks, blocks.data(), sizeof(pv::VarBlock) * blocks.size(), hipMemcpyHostToDevice));
    PV_HIP(hipMemcpy(vr->d_tiles, tiles.data(), sizeof(pv::VarTile) * tiles.size(), hipMemcpyHostToDevice));
    PV_HIP(hipDeviceSynchronize());
    vr->copy = 0;
    vr->copy_shift = 0;
    vr->span4_max = span4_max;
    vr->nblocks = nblocks;
    return PV_OK;
}

long long pv_varresample_length(const pv_varresampler* vr) { return vr ? (long long)vr->nblocks * vr->block : 0; }

pv_status pv_varresample(pv_varresampler* vr, const float* x, long long ldx, long long n_in, int channels, float* y,
                         long long ldy, long long n_out, void* stream) {
    if (!vr) return fail(PV_ERR_ARG, "null variable-rate resampler");
    if (channels < 0 || n_in < 0 || n_out < 0) return fail(PV_ERR_ARG, "negative channels / n_in / n_out");
    if (vr->nblocks < 1) return fail(PV_ERR_ARG, "pv_varresample: no map (pv_varresampler_set_map first)");
    if (n_out > pv_varresample_length(vr)) return fail(PV_ERR_ARG, "pv_varresample: n_out > pv_varresample_length");
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
    const long long rows = pv_output_length(h, std::max(h->cfg.max_frames, 1));
    // (rows of a multiple of 4 floats, shared with pv_pitch_reserve: whichever comes first allocates)
    if (!h->d_pitch) {
        const long long ld = (rows + 3) & ~3LL;
        if (h->d_pitch.alloc((size_t)ld * (size_t)std::max(h->cfg.max_channels, 1)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PV_ERR_NOMEM, "pv_pitchmap_set: scratch rows");
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
        st = pv_varresampler_create(quality, h->hop, (int)max_blocks, h->cfg.device, &h->pmap_vr);
        if (st != PV_OK) return st;
    }
    st = pv_varresampler_set_map(h->pmap_vr, 0, step.data(), (int)step.size());
    if (st == PV_OK) st = timemap_set("pv_pitchmap_set", h, pos_s.data(), (int)pos_s.size());
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
