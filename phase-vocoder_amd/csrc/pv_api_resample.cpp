// pv_api_resample.cpp — the resampler of libpv and the pitch shift built on it.
// pv_resampler (pv_host.hpp): a reduced ratio P:Q, a quality preset and the polyphase
// coefficient table in device memory (pv_resample.hpp; the coefficients are pv_tables.cpp's);
// pv_pitch_process: a STANDARD time stretch into the handle's scratch rows, resampled by
// out_hop : hop.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pv_host.hpp"

namespace pvhost {

namespace {
// the eight alignments of the Q x 2W coefficient table (pv_resample.hpp ResampleParams::tab)
void resample_table(int P, int Q, int quality, const pv::ResamplePlan& plan, std::vector<float>& tab) {
    const int W = plan.W, NC = plan.NC;
    std::vector<float> row(2 * W);
    tab.assign((size_t)8 * Q * NC * 4, 0.0f);
    for (int r = 0; r < Q; ++r) {
        resample_row(P, Q, quality, W, r, row.data());
        for (int off = 0; off < 8; ++off) {
            float* dst = tab.data() + ((size_t)off * Q + r) * NC * 4;
            for (int t = 0; t < 2 * W; ++t) dst[t + off] = row[t];
        }
    }
}
}  // namespace

hipError_t resample_rows(const pv_resampler* rs, const float* x, long long ldx, long long n_in, int channels,
                         float* y, long long ldy, hipStream_t s) {
    if (!rs->d_tab) return pv::launch_copy_rows(x, ldx, y, ldy, n_in, channels, s);
    pv::ResampleParams p{};
    p.x = x;
    p.ldx = ldx;
    p.n_in = n_in;
    p.y = y;
    p.ldy = ldy;
    p.n_out = resample_length(rs->P, rs->Q, n_in);
    p.tab = rs->d_tab;
    p.P = rs->P;
    p.Q = rs->Q;
    p.plan = rs->plan;
    const long long T = (long long)rs->plan.R * rs->plan.D;
    const long long ntiles = (p.n_out + T - 1) / T;
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;
    p.ntiles = (int)ntiles;
    return pv::launch_resample(channels, p, s);
}

}  // namespace pvhost

using namespace pvhost;

extern "C" {

pv_status pv_resampler_create(int p, int q, int quality, int device, pv_resampler** out) {
    if (!out) return fail(PV_ERR_ARG, "null argument");
    *out = nullptr;
    if (p <= 0 || q <= 0) return fail(PV_ERR_ARG, "pv_resampler_create: p and q must be positive");
    pv_status st = check_quality("pv_resampler_create", quality);
    if (st != PV_OK) return st;
    const long long g = gcd_ll(p, q);
    const long long P = p / g, Q = q / g;
    if (P > 4096 || Q > 4096 || P > 4 * Q || Q > 4 * P)
        return fail(PV_ERR_UNSUPPORTED, "pv_resampler_create: ratio in [1/4, 4] with reduced p, q <= 4096");
    std::unique_ptr<pv_resampler> rs(new pv_resampler());  // (no table yet: nothing to free on a device)
    rs->P = (int)P;
    rs->Q = (int)Q;
    rs->quality = quality;
    rs->device = device;
    if (P != Q) {
        const int W = resample_half_width(rs->P, rs->Q, quality);
        if (!pv::resample_plan(rs->P, rs->Q, W, &rs->plan))
            return fail(PV_ERR_UNSUPPORTED, "pv_resampler_create: no tile plan for this ratio");
        std::vector<float> tab;
        resample_table(rs->P, rs->Q, quality, rs->plan, tab);
        DeviceGuard dg(device);
        DevBuf<float4> d_tab;
        if (d_tab.alloc(tab.size() / 4) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PV_ERR_NOMEM, "pv_resampler_create: coefficient table");
        }
        if (hipMemcpy(d_tab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(PV_ERR_HIP, "pv_resampler_create: uploading the coefficient table");
        rs->d_tab = std::move(d_tab);
    }
    *out = rs.release();
    return PV_OK;
}

void pv_resampler_destroy(pv_resampler* rs) {
    if (!rs) return;
    if (rs->d_tab) {
        DeviceGuard dg(rs->device);
        rs->d_tab.reset();
    }
    delete rs;
}

long long pv_resample_length(const pv_resampler* rs, long long n_in) {
    return rs ? resample_length(rs->P, rs->Q, n_in) : 0;
}

pv_status pv_resample(pv_resampler* rs, const float* x, long long ldx, long long n_in, int channels, float* y,
                      long long ldy, void* stream) {
    if (!rs) return fail(PV_ERR_ARG, "null resampler");
    if (channels < 0 || n_in < 0) return fail(PV_ERR_ARG, "negative channels / n_in");
    if (channels == 0 || n_in == 0) return PV_OK;
    if (!x || !y) return fail(PV_ERR_ARG, "null x/y");
    const long long n_out = resample_length(rs->P, rs->Q, n_in);
    if (channels > 1 && (ldx < n_in || ldy < n_out)) return fail(PV_ERR_ARG, "ldx < n_in or ldy < pv_resample_length");
    const float* xe = x + (channels - 1) * ldx + n_in;
    const float* ye = y + (channels - 1) * ldy + n_out;
    if ((uintptr_t)x < (uintptr_t)ye && (uintptr_t)y < (uintptr_t)xe) return fail(PV_ERR_ARG, "x and y overlap");
    DeviceGuard dg(rs->device);
    const hipError_t e = resample_rows(rs, x, ldx, n_in, channels, y, ldy, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("resample launch: ") + hipGetErrorString(e));
    return PV_OK;
}

pv_status pv_pitch_reserve(pv_handle* h, int quality) {
    if (!h) return fail(PV_ERR_ARG, "null handle");
    pv_status st = check_std_stretch("pv_pitch_reserve", h);
    if (st != PV_OK || (st = check_quality("pv_pitch_reserve", quality)) != PV_OK) return st;
    pv_resampler* rs = nullptr;
    st = pv_resampler_create(h->hs, h->hop, quality, h->cfg.device, &rs);
    if (st != PV_OK) return st;
    DeviceGuard g(h->cfg.device);
    // (rows of a multiple of 4 floats; a repeated reserve keeps the rows it has)
    if (!h->d_pitch) {
        const long long ld = (pv_output_length(h, std::max(h->cfg.max_frames, 1)) + 3) & ~3LL;
        if (h->d_pitch.alloc((size_t)ld * (size_t)std::max(h->cfg.max_channels, 1)) != hipSuccess) {
            (void)hipGetLastError();
            pv_resampler_destroy(rs);
            return fail(PV_ERR_NOMEM, "pv_pitch_reserve: scratch rows");
        }
        h->ld_pitch = ld;
    }
    if (h->pitch_rs) {
        (void)hipDeviceSynchronize();  // calls in flight read the old table
        pv_resampler_destroy(h->pitch_rs);
    }
    h->pitch_rs = rs;
    return PV_OK;
}

long long pv_pitch_output_length(const pv_handle* h, int frames) {
    if (!h) return 0;
    return resample_length(h->hs, h->hop, pv_output_length(h, frames));
}

pv_status pv_pitch_process(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels,
                           int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                           void* stream) {
    pv_status st = check_common(h, channels, frames);
    if (st != PV_OK) return st;
    if (!h->pitch_rs) return fail(PV_ERR_ARG, "pv_pitch_process: call pv_pitch_reserve first");
    DeviceGuard g(h->cfg.device);
    ProfCall pc_(h);
    hipStream_t s = (hipStream_t)stream;
    // out hop = hop: no resampling, the time stretch writes `out`
    if (!h->pitch_rs->d_tab)
        return process_impl(h, x, ldx, n_samples, channels, frames, spec, ld_spec, out, ldo, s);
    if (channels == 0 || frames == 0) return PV_OK;
    if (!out) return fail(PV_ERR_ARG, "null out");
    const long long n_mid = pv_output_length(h, frames);
    if (channels > 1 && ldo < resample_length(h->pitch_rs->P, h->pitch_rs->Q, n_mid))
        return fail(PV_ERR_ARG, "ldo < pv_pitch_output_length");
    st = process_impl(h, x, ldx, n_samples, channels, frames, spec, ld_spec, h->d_pitch, h->ld_pitch, s);
    if (st != PV_OK) return st;
    PV_LAUNCH(h, KRES, s, resample_rows(h->pitch_rs, h->d_pitch, h->ld_pitch, n_mid, channels, out, ldo, s));
    return PV_OK;
}

}  // extern "C"
