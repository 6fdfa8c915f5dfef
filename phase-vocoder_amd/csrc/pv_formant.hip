// pv_formant.hip — formant-preserving STANDARD pitch shift (pv_set_formant).
//
//   k_envelope            per frame: lg = ln max(mag, 2^-30) -> cepstrum (inverse real FFT) ->
//                         lifter |quefrency| <= order -> log envelope le (forward real FFT,
//                         real part) -> one fp32 row per frame
//   k_synthesis           K3 of the pitch shift: the instantiations of k_synthesis
//                         (pv_syn_kernel.hpp) in the formant mode and their launch.  The frames
//                         gather mag exp(-le) and re-colour the sum with exp(le) of the target
//                         bin (synth_frame's kModeFormant, formant_gather in pv_formant.hpp)
//
// Neither keeps state across frames: the unwrap state, the carries, the run records and the
// stream segments are those of the plain pitch shift.  A translation unit of its own: the
// kernels compile next to the other modes', and their registers are checked file by file
// (tests/test_formant_ref.py).
#include "pv_syn_kernel.hpp"

namespace pv {

// ------------------------------------------------------------------ envelope
// One wave per run of F frames (the synthesis's runs), a workgroup of 4 runs.  The wave holds
// a frame as everywhere: bin k = lane + 64 i in slot i, bin L in slot E.  Both transforms are
// the L-point complex FFT of the real-FFT pair the synthesis and the analysis use, in the
// twiddle-first radix-E form (fft_pass_v3) on one pass table: the inverse through synth_frame's
// MODE 5 (Y = lg + 0 i: pre-step + inverse FFT, unnormalised: N c[n]), whose last pass leaves
// the time samples 2 m, 2 m + 1 (m = lane + 64 last_slot) in the registers, where the lifter
// and the 1 / N are applied; those registers, renamed, are the forward FFT's input layout.
// The forward transform's natural-order image goes through the tile, and the real split keeps
// the real part (the cepstrum is real and even: Im rfft(c) is rounding).
constexpr float kFormantFloor = 0x1p-30f;

template <int L>
__global__ __launch_bounds__(256, (L <= 256) ? 4 : (L == 512) ? 3 : 2) void k_envelope(EnvParams p) {
    using G_ = Geo<L>;
    constexpr int E = G_::E;
    constexpr int N = 2 * L;
    constexpr bool V3X = (L == 1024);
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

    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    const int t0 = run * p.F;
    const int nfr = max(0, min(p.F, p.frames - t0));
    const float2* specc = p.spec + (long long)c * p.ld_spec;
    float* envc = p.env + (long long)c * p.ld_env;
    const bool packed = p.packed != 0;
    const int order = p.order;

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
        // lg = ln max(mag, 2^-30): maxNum (a NaN magnitude gives the floor), hardware log2
        float2 sv[E + 1];
#pragma unroll
        for (int i = 0; i <= E; ++i)
            sv[i] = make_float2(__builtin_amdgcn_logf(__builtin_fmaxf(mag[i], kFormantFloor)) * kLn2, 0.0f);
        float2 z[E];
        synth_frame<L, 5, false, false, false, false, false, NoHook, NoTwReg, V3X>(
            sv, false, 0u, M, phprev, pmap, stb, tw0, tile, lane, z, ekr, jkr);
        // lifter and 1 / N on the time samples n = 2 m + {0, 1}: kept iff min(n, N - n) <= order
        float2 v[E];
        static_for<0, E>([&](auto ic) {
            constexpr int idx = decltype(ic)::value;
            constexpr int cs = last_slot<L>(idx);
            const int n0 = 2 * (lane + 64 * cs), n1 = n0 + 1;
            constexpr float inv_n = 1.0f / (float)N;
            v[cs] = make_float2(min(n0, N - n0) <= order ? z[idx].x * inv_n : 0.0f,
                                min(n1, N - n1) <= order ? z[idx].y * inv_n : 0.0f);
        });
        fft_run<L, false, true, 0, 0, V3X>(v, tile, twl, tw0, lane);
        // real part of the real split (split_chunk_bp's operations), bins lane + 64 i and L
        float2 A[E + 1], Bz[E + 1], tw[E + 1];
#pragma unroll
        for (int i = 0; i <= E; ++i) {
            const int k = (i == E) ? L : lane + 64 * i;
            A[i] = lds_ld(&tile[k & (L - 1)]);
            Bz[i] = lds_ld(&tile[(L - k) & (L - 1)]);
            tw[i] = lds_ld(&twsl[k]);
        }
        wave_lds_sync();  // the next frame's first tile store stays after these reads
        float* erow = envc + (long long)t * p.env_stride;
        float leL = 0.0f;
#pragma unroll
        for (int i = 0; i <= E; ++i) {
            const float er = 0.5f * (A[i].x + Bz[i].x);
            const float orr = 0.5f * (A[i].y + Bz[i].y);
            const float oi = 0.5f * (Bz[i].x - A[i].x);
            const float le = __builtin_fmaf(orr, tw[i].x, __builtin_fmaf(-oi, tw[i].y, er));
            if (i < E) erow[lane + 64 * i] = le;
            else leL = le;
        }
        // bin L and the row's padding (env_tail slots from L on, all inside the row)
        if (lane < p.env_tail) erow[L + lane] = (lane == 0) ? leL : 0.0f;
    }
}

template <int L>
static size_t env_lds() { return sizeof(float2) * (L + (L + 2) + 4 * Geo<L>::TILE); }

hipError_t launch_envelope(int L, int channels, const EnvParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    switch (L) {
        case 128: hipLaunchKernelGGL(k_envelope<128>, grid, dim3(256), env_lds<128>(), s, p); break;
        case 256: hipLaunchKernelGGL(k_envelope<256>, grid, dim3(256), env_lds<256>(), s, p); break;
        case 512: hipLaunchKernelGGL(k_envelope<512>, grid, dim3(256), env_lds<512>(), s, p); break;
        case 1024: hipLaunchKernelGGL(k_envelope<1024>, grid, dim3(256), env_lds<1024>(), s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ K3, formant mode
// the kernel of launch_synthesis's mode 2 for the same geometry (launch_syn_plain), up to
// L = 1024; one kernel per geometry serves ratios above and below 1
hipError_t launch_synthesis_formant(int L, int channels, const SynParams& p, hipStream_t s) {
    if (!p.env) return hipErrorInvalidValue;
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    const int dt = qp ? syn_dt(L, p.hs) : 0;
    return qp ? launch_syn_plain<kModeFormant, true, 1024>(L, dt, grid, p, s)
              : launch_syn_plain<kModeFormant, false, 1024>(L, dt, grid, p, s);
}

}  // namespace pv
