// pv_warp.hip — K3 of the STANDARD time stretch with the envelope warp (pv_pitch_set_formant;
// DESIGN.md §3.10): formant preservation for the stretch-and-resample pitch shift.  The split
// synthesis of pv_kernels.hip — one wave per run of F frames, a workgroup of 4 consecutive
// runs, register or LDS-ring overlap-add, seam tails for k_seam — whose frames scale every
// magnitude by exp(lw - le): the frame's log envelope (k_envelope's row, loaded one frame ahead
// like k_synthesis_formant's) read at the bin's warp position (synth_frame's kModeWarp /
// kModeLockedWarp, warp_gains in pv_warp.hpp).  LOCK: the output phases are the locked stretch's
// (lock_offsets), with every peak and owner decision made on the unscaled magnitudes.
//
// The unwrap state, the carries, the run records and the stream segments are those of the
// plain stretch: the warp adds no state across frames.  A kernel of its own, so that the tuned
// k_synthesis and k_synthesis_locked instantiations keep their code.  No per-lane-constant
// (LANEK), partial-row (NR) or self-tracked-prefetch variants.
#include "pv_syn_run.hpp"

namespace pv {

// waves per SIMD the kernels are compiled for: as k_synthesis_formant (L = 512 at 2 and
// L = 1024 at 1: up to 256 VGPRs; the envelope row and its prefetch sit next to the spectrum
// row, the peak words of the locked form next to both)
template <int L, bool LOCK, int DT, bool QPOW2>
__global__ __launch_bounds__(256, (L <= 256) ? 4 : (L == 512) ? 2 : 1) void k_synthesis_warp(SynParams p) {
    constexpr int MODE = LOCK ? kModeLockedWarp : kModeWarp;
    using G_ = Geo<L>;
    using T_ = SynTraits<L, MODE, DT, QPOW2>;
    constexpr bool ROLA = DT > 0;
    constexpr int E = G_::E;
    constexpr int N = 2 * L;
    constexpr int B = L + 1;
    constexpr bool GREG = T_::GREG;  // ROLA gains in registers (else LDS)
    constexpr bool RACC = T_::RACC;
    constexpr int NS = T_::NS, D = T_::D;
    // the LDS carve-up of k_synthesis (syn_lds): tables, 4 tiles, rings / gains, unwrap constants,
    // and the warp map where the pitch shift keeps its bin map
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2* twl = reinterpret_cast<float2*>(smem);                     // L
    float2* twsl = twl + L;                                            // L (+2 pad)
    float2* tiles = twsl + (L + 2);                                    // 4 x TILE
    float* after_tiles = reinterpret_cast<float*>(tiles + 4 * G_::TILE);
    float* rings = ROLA ? reinterpret_cast<float*>(tiles) : after_tiles;  // ROLA: tails, after the loop
    float* gainl = ROLA ? after_tiles : rings + 4 * N;                 // N (unless GREG)
    float* ekl = gainl + (GREG ? 0 : N);                               // B (+pad)
    unsigned* jkl = reinterpret_cast<unsigned*>(ekl + (B + 3));        // B (+pad)
    int* srcl = reinterpret_cast<int*>(jkl + (B + 3));                 // 2 x B {i_k, bits of f_k}
    const int hs = p.hs;
    const int TL = N - hs;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2 tw0[E];
    load_tw0<L>(tw0, p.tw);
    for (int i = tid; i < L; i += 256) { twl[i] = p.tw[i]; twsl[i] = p.tws[i]; }
    if (!GREG)
        for (int i = tid; i < N; i += 256) gainl[i] = p.gain[i];
    for (int i = tid; i < B; i += 256) {
        ekl[i] = p.ek[i];
        // RACC: (p j_k mod q) / q as a float (exact: q <= 4096)
        jkl[i] = RACC ? __float_as_uint((float)p.jk_mod[i] * p.inv_q) : p.jk_mod[i];
        // the warp map travels in the pitch map's fields (a time stretch has no bin map)
        srcl[2 * i] = p.src_first[i];
        srcl[2 * i + 1] = p.src_cnt[i];
    }
    float* ring = rings + w * N;
    if (!ROLA) {
#pragma unroll
        for (int i = 0; i < N / 64; ++i) ring[lane + 64 * i] = 0.0f;
    }
    __syncthreads();

    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    const int t0 = run * p.F;
    const int nfr = max(0, min(p.F, p.frames - t0));  // real frames of this wave's run
    float* outc = p.out + (long long)c * p.ldo;
    const long long obase = (long long)t0 * hs;

    int M[E + 1];
    float phprev[E + 1];
    if (nfr > 0) {
        // no carries when the output phase does not depend on the unwrap count (q = 1)
        const int* cr = p.carry ? p.carry + ((long long)c * p.nruns + run) * p.bins_pad : nullptr;
        if constexpr (RACC) {
            const unsigned qm = (unsigned)p.q - 1u;
            PV_FOR_BINS(E, lane, {
                const unsigned mq = cr ? ((unsigned)p.p_mod * ((unsigned)cr[k] & qm)) & qm : 0u;
                M[i] = __float_as_int((float)mq * p.inv_q);
                phprev[i] = 0.0f;
            })
        } else {
            PV_FOR_BINS(E, lane, { M[i] = cr ? cr[k] : 0; phprev[i] = 0.0f; })
        }
    }
    float2 acc[NS];
    syn_run<L, MODE, DT, QPOW2>(p, SynCarve{twl, twsl, tiles, rings, gainl, ekl, jkl, srcl}, tw0, lane, w, c, t0, nfr,
                                M, phprev, acc);
    if constexpr (ROLA) {
        // the run's tail (positions F*hs + j, j < N - hs) -> ring[j], over the tiles
        __syncthreads();
        float2* r2 = reinterpret_cast<float2*>(ring);
#pragma unroll
        for (int s = 0; s < NS - D; ++s) r2[64 * s + lane] = acc[s];
    }
    __syncthreads();
    // seams, as k_synthesis: run w's tail (positions F*hs + j) overlaps run w+1's head, which
    // that run has stored; the workgroup's last tail goes to `tails` for k_seam, or to `out`
    // at the end of the channel.  Every access is bounds-checked against out_len.
    const int nwg = (p.nruns + 3) / 4;
    const bool last = (blockIdx.x + 1 >= nwg);
    if (w > 0) {
        const float* prev = rings + (w - 1) * N;
        for (int j = lane; j < TL; j += 64) {
            const long long gp = obase + j;
            if (gp < p.out_len) outc[gp] += prev[ROLA ? j : ((p.F * hs + j) & (N - 1))];
        }
    }
    if (w == 3) {
        float* tdst = p.tails + ((long long)c * nwg + blockIdx.x) * p.tail_len;
        for (int j = lane; j < TL; j += 64) {
            const float v = ring[ROLA ? j : ((p.F * hs + j) & (N - 1))];
            if (last) {
                const long long gp = obase + (long long)p.F * hs + j;
                if (gp < p.out_len) outc[gp] = v;
            } else {
                tdst[j] = v;
            }
        }
    }
}

// the kernel of launch_synthesis_locked for the same geometry: register overlap-add (out hop
// 128, 256 or 512) where q is a power of two <= 4096, the LDS ring otherwise
template <bool LOCK, bool QP>
static hipError_t launch_warp_q(int L, int dt, dim3 grid, const SynParams& p, hipStream_t s) {
#define PV_WARP_DT(LL_, DT_) \
    hipLaunchKernelGGL((k_synthesis_warp<LL_, LOCK, DT_, QP>), grid, dim3(256), syn_lds<LL_>(DT_), s, p)
#define PV_WARP_L(LL_)                                   \
    if constexpr (QP) {                                  \
        switch (dt) {                                    \
            case 1: PV_WARP_DT(LL_, 1); break;           \
            case 2: PV_WARP_DT(LL_, 2); break;           \
            case 4: PV_WARP_DT(LL_, 4); break;           \
            default: PV_WARP_DT(LL_, 0); break;          \
        }                                                \
    } else {                                             \
        PV_WARP_DT(LL_, 0);                              \
    }
    switch (L) {
        case 128: PV_WARP_L(128); break;
        case 256: PV_WARP_L(256); break;
        case 512: PV_WARP_L(512); break;
        case 1024: PV_WARP_L(1024); break;
        default: return hipErrorInvalidValue;
    }
#undef PV_WARP_L
#undef PV_WARP_DT
    return hipGetLastError();
}

hipError_t launch_synthesis_warp(int L, int lock, int channels, const SynParams& p, hipStream_t s) {
    if (!p.env || !p.src_first || !p.src_cnt) return hipErrorInvalidValue;
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    const int dt = qp ? syn_dt(L, p.hs) : 0;
    if (lock) return qp ? launch_warp_q<true, true>(L, dt, grid, p, s) : launch_warp_q<true, false>(L, dt, grid, p, s);
    return qp ? launch_warp_q<false, true>(L, dt, grid, p, s) : launch_warp_q<false, false>(L, dt, grid, p, s);
}

}  // namespace pv
