// pv_pitchtrack.hip — the pitch tracker (pv_pitch_track).
//
//   k_pitch   per frame: P = (mag s)^2 with s the power of two that brings the frame's largest
//             magnitude into [1, 2) -> circular autocorrelation r (inverse real FFT) ->
//             rho[n] = r[n] / (r[0] g[n]), g the periodic Hann's own autocorrelation ->
//             the smallest local maximum within kappa of the largest, over the lags
//             tau_min .. tau_max -> a parabola through its neighbours -> {f0, strength}
//
// No state across frames, no table of its own, nothing allocated: capturable from the first
// call.  A translation unit of its own: every other kernel keeps its instructions.
#include "pv_pitchtrack.hpp"
#include "pv_syn_kernel.hpp"

namespace pv {

// One wave per run of F frames, a workgroup of 4 runs: k_envelope's frame and LDS structure.
// The wave holds a frame as everywhere: bin k = lane + 64 i in slot i, bin L in slot E.  The
// inverse transform is synth_frame's MODE 5 (Y = P + 0 i: pre-step + inverse FFT, unnormalised:
// N r[n]), whose last pass leaves the lags 2 m, 2 m + 1 (m = lane + 64 last_slot) in the
// registers.  Only the lags 0 .. L are used: last slots 0 .. E/2 - 1, and lag L in slot E/2 of
// lane 0 (the other lags of that slot, L + 2 .. L + 127, ride along and are never read).
// 1 / g of the lane's own lags is computed once per wave (v_cos_f32 on the exact fraction n / N,
// one IEEE division each).  rho goes to the wave's tile as N floats, rho[n] at float n; a lag's
// neighbours come back from there, and so do the three values around the pick (one address on
// every lane).  The maximum of the magnitudes, the largest candidate and the smallest qualifying
// lag are butterflies over the lanes.  Every division is IEEE (one per frame each: 1 / r[0], the
// parabola's offset, 1 / (tau + d)); a lag costs two multiplies.
template <int L>
__global__ __launch_bounds__(256, (L <= 256) ? 4 : (L == 512) ? 3 : 2) void k_pitch(PitchParams p) {
    using G_ = Geo<L>;
    constexpr int E = G_::E;
    constexpr int N = 2 * L;
    constexpr int H = E / 2;
    constexpr bool V3X = (L == 1024);
    static_assert(2 * G_::TILE >= L + 128, "the tile holds rho of the lags 0 .. L + 127");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2* twl = reinterpret_cast<float2*>(smem);  // L
    float2* twsl = twl + L;                         // L + 1 (+1 pad)
    float2* tiles = twsl + (L + 2);                 // 4 x TILE
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < L; i += 256) twl[i] = p.tw[i];
    for (int i = tid; i <= L; i += 256) twsl[i] = p.tws[i];
    __syncthreads();
    float2* tile = tiles + w * G_::TILE;
    float* rho = reinterpret_cast<float*>(tile);

    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    const int t0 = run * p.F;
    const int nfr = max(0, min(p.F, p.frames - t0));
    const float2* specc = p.spec + (long long)c * p.ld_spec;
    float2* dstc = p.dst + (long long)c * p.ld_dst;
    const bool packed = p.packed != 0;
    const int tau_min = p.tau_min, tau_max = p.tau_max;
    const float kappa = p.kappa;

    // (the v3 passes take every twiddle from the pass table: tw0 and the unwrap arguments of
    // synth_frame are not used by MODE 5)
    float2 tw0[E];
#pragma unroll
    for (int i = 0; i < E; ++i) tw0[i] = make_float2(1.0f, 0.0f);
    int M[E + 1];
    float phprev[E + 1], ekr[E + 1];
    unsigned jkr[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) { M[i] = 0; phprev[i] = 0.0f; ekr[i] = 0.0f; jkr[i] = 0u; }
    const PhaseMap pmap{0.0f, 1u, 0u, 1, 1.0f, 0.0f, 0};
    const SynLds stb{twl, twsl, nullptr, nullptr, nullptr};

    // 1 / g[n] = 3 / (2 + cos(2 pi n / N)) of the lags 2 m, 2 m + 1, m = lane + 64 cs, cs <= H
    float2 invg[H + 1];
#pragma unroll
    for (int cs = 0; cs <= H; ++cs) {
        const int n0 = 2 * (lane + 64 * cs);
        constexpr float inv_n = 1.0f / (float)N;
        invg[cs] = make_float2(3.0f / (2.0f + __builtin_amdgcn_cosf((float)n0 * inv_n)),
                               3.0f / (2.0f + __builtin_amdgcn_cosf((float)(n0 + 1) * inv_n)));
    }

    // the row one frame ahead; every lane reads bin L's slot (one address; packed rows: slot 0)
    float2 nx[E + 1];
    auto load_row = [&](const float2* srow) {
#pragma unroll
        for (int i = 0; i < E; ++i) nx[i] = srow[lane + 64 * i];
        nx[E] = srow[packed ? 0 : L];
    };
    if (nfr > 0) load_row(specc + (long long)t0 * p.spec_stride);
    for (int u = 0; u < nfr; ++u) {
        const int t = t0 + u;
        float mag[E + 1];
#pragma unroll
        for (int i = 0; i <= E; ++i) mag[i] = nx[i].x;
        if (packed) {
            // PV_SPEC_PACKED slot 0 = {s0, sL}: the magnitudes are the sign-free values
            float2 b0, bl;
            unpack_real_bins(nx[E], b0, bl);
            mag[E] = bl.x;
            if (lane == 0) mag[0] = b0.x;
        }
        if (u + 1 < nfr) load_row(specc + (long long)(t + 1) * p.spec_stride);
        float2 res = make_float2(0.0f, 0.0f);
        // the frame's largest magnitude: maxNum (a NaN magnitude counts as 0), every lane's
        // slot E holds bin L
        float mx = 0.0f;
#pragma unroll
        for (int i = 0; i <= E; ++i) mx = __builtin_fmaxf(mx, mag[i]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, d));
        const unsigned mxb = __builtin_amdgcn_readfirstlane(__float_as_uint(mx));
        if (mxb != 0u && mxb < 0x7f800000u) {
            // s = 2^-exponent(mx) from mx's bits (the exponent taken as at most 126, so that s is
            // a normal number): mag s is exact, and a power-of-two scaling of the input drops out
            const int sbe = max(254 - (int)(mxb >> 23), 1);
            const float s = __uint_as_float((unsigned)sbe << 23);
            float2 sv[E + 1];
#pragma unroll
            for (int i = 0; i <= E; ++i) {
                const float a = __builtin_fmaxf(mag[i], 0.0f) * s;
                sv[i] = make_float2(a * a, 0.0f);
            }
            float2 z[E];
            synth_frame<L, 5, false, false, false, false, false, NoHook, NoTwReg, V3X>(
                sv, false, 0u, M, phprev, pmap, stb, tw0, tile, lane, z, ekr, jkr);
            // N r[0]: lane 0's last slot 0
            const float r0 = __uint_as_float(
                __builtin_amdgcn_readfirstlane(__float_as_uint(z[slot_reg<L>(0)].x)));
            if (r0 > 0.0f) {
                const float inv0 = 1.0f / r0;
                float2 rh[H];
                static_for<0, E>([&](auto ic) {
                    constexpr int idx = decltype(ic)::value;
                    constexpr int cs = last_slot<L>(idx);
                    if constexpr (cs <= H) {
                        const float2 v = make_float2((z[idx].x * inv0) * invg[cs].x, (z[idx].y * inv0) * invg[cs].y);
                        tile[lane + 64 * cs] = v;
                        if constexpr (cs < H) rh[cs] = v;
                    }
                });
                wave_lds_sync();
                // candidates among the lane's own lags; top: the largest candidate's rho
                bool cand[H][2];
                float top = 0.0f;
#pragma unroll
                for (int cs = 0; cs < H; ++cs) {
                    const int n0 = 2 * (lane + 64 * cs), n1 = n0 + 1;
                    const float lo = lds_ld(&rho[max(n0 - 1, 0)]);
                    const float hi = lds_ld(&rho[n1 + 1]);
                    const float a = rh[cs].x, b = rh[cs].y;
                    cand[cs][0] = n0 >= tau_min && n0 <= tau_max && a > lo && a >= b && a > 0.0f;
                    cand[cs][1] = n1 >= tau_min && n1 <= tau_max && b > a && b >= hi && b > 0.0f;
                    if (cand[cs][0]) top = __builtin_fmaxf(top, a);
                    if (cand[cs][1]) top = __builtin_fmaxf(top, b);
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) top = __builtin_fmaxf(top, __shfl_xor(top, d));
                if (__builtin_amdgcn_readfirstlane(__float_as_uint(top)) != 0u) {
                    // the key maximum: the smallest candidate within kappa of the largest
                    const float thr = kappa * top;
                    int tau = N;
#pragma unroll
                    for (int cs = 0; cs < H; ++cs) {
                        const int n0 = 2 * (lane + 64 * cs), n1 = n0 + 1;
                        if (cand[cs][1] && rh[cs].y >= thr) tau = min(tau, n1);
                        if (cand[cs][0] && rh[cs].x >= thr) tau = min(tau, n0);
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) tau = min(tau, __shfl_xor(tau, d));
                    tau = __builtin_amdgcn_readfirstlane(tau);
                    // (the largest candidate qualifies: kappa <= 1, and a product rounds monotonically)
                    tau = min(tau, L - 1);
                    const float a = lds_ld(&rho[tau - 1]), b = lds_ld(&rho[tau]), cc = lds_ld(&rho[tau + 1]);
                    // b > a and b >= cc: the curvature is below zero, exactly
                    const float den = (a - b) + (cc - b);
                    const float d = (0.5f * (a - cc)) / den;
                    res = make_float2(1.0f / ((float)tau + d), b - (0.25f * (a - cc)) * d);
                }
                wave_lds_sync();  // the next frame's first tile store stays after these reads
            }
        }
        if (lane == 0) dstc[t] = res;
    }
}

template <int L>
static size_t pitch_lds() { return sizeof(float2) * (L + (L + 2) + 4 * Geo<L>::TILE); }

hipError_t launch_pitch(int L, int channels, const PitchParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    switch (L) {
        case 128: hipLaunchKernelGGL(k_pitch<128>, grid, dim3(256), pitch_lds<128>(), s, p); break;
        case 256: hipLaunchKernelGGL(k_pitch<256>, grid, dim3(256), pitch_lds<256>(), s, p); break;
        case 512: hipLaunchKernelGGL(k_pitch<512>, grid, dim3(256), pitch_lds<512>(), s, p); break;
        case 1024: hipLaunchKernelGGL(k_pitch<1024>, grid, dim3(256), pitch_lds<1024>(), s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pv
