// pv_locked.hip — K3 of the STANDARD time stretch with identity phase locking
// (pv_set_phase_lock): the split synthesis of pv_kernels.hip — one wave per
// run of F frames, a workgroup of 4 consecutive runs, register or LDS-ring overlap-add, seam
// tails for k_seam (syn_workgroup, pv_syn_run.hpp) — whose frames take every bin's output phase
// from the magnitude peak that owns the bin (synth_frame's kModeLocked, lock_offsets in
// pv_lock.hpp).  The unwrap state, the carries, the run records and the stream segments are
// those of the unlocked path: locking adds no state across frames.
//
// A kernel of its own, so that the tuned k_synthesis instantiations keep their registers and
// occupancy.  It has no per-lane-constant (LANEK) or partial-row (NR) variants.
#include "pv_syn_run.hpp"

namespace pv {

// waves per SIMD the kernels are compiled for: as k_synthesis up to L = 256 and at L >= 1024
// (1: the compiler may use up to 256 VGPRs, the LDS sets the occupancy); L = 512 at 2 (256
// VGPRs): the peak words and the owner search do not fit the 168 of k_synthesis's 3 without
// spills, which the self-tracked row prefetch of that size cannot have (syn_run FASTOK)
template <int L, int DT, bool QPOW2>
__global__ __launch_bounds__(256, (L <= 256) ? 4 : (L == 512) ? 2 : 1) void k_synthesis_locked(SynParams p) {
    using G_ = Geo<L>;
    using T_ = SynTraits<L, kModeLocked, DT, QPOW2>;
    constexpr bool ROLA = DT > 0;
    constexpr int E = G_::E;
    constexpr int N = 2 * L;
    constexpr int B = L + 1;
    constexpr bool GREG = T_::GREG;  // ROLA gains in registers (else LDS)
    constexpr bool RACC = T_::RACC;
    constexpr int NS = T_::NS, D = T_::D;
    // the LDS carve-up of k_synthesis (syn_lds): tables, 4 tiles, rings / gains, unwrap constants
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2* twl = reinterpret_cast<float2*>(smem);                     // L
    float2* twsl = twl + L;                                            // L (+2 pad)
    float2* tiles = twsl + (L + 2);                                    // 4 x TILE
    float* after_tiles = reinterpret_cast<float*>(tiles + 4 * G_::TILE);
    float* rings = ROLA ? reinterpret_cast<float*>(tiles) : after_tiles;  // ROLA: tails, after the loop
    float* gainl = ROLA ? after_tiles : rings + 4 * N;                 // N (unless GREG)
    float* ekl = gainl + (GREG ? 0 : N);                               // B (+pad)
    unsigned* jkl = reinterpret_cast<unsigned*>(ekl + (B + 3));        // B (+pad)
    int* srcl = reinterpret_cast<int*>(jkl + (B + 3));                 // (pitch map: unused)
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
    syn_run<L, kModeLocked, DT, QPOW2>(p, SynCarve{twl, twsl, tiles, rings, gainl, ekl, jkl, srcl}, tw0, lane, w, c,
                                       t0, nfr, M, phprev, acc);
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

// the kernel of launch_synthesis's mode 0 for the same geometry: register overlap-add
// (out hop 128, 256 or 512, L <= 1024) where q is a power of two <= 4096, the LDS ring otherwise
template <bool QP>
static hipError_t launch_locked_q(int L, int dt, dim3 grid, const SynParams& p, hipStream_t s) {
#define PV_LOCK_DT(LL_, DT_) \
    hipLaunchKernelGGL((k_synthesis_locked<LL_, DT_, QP>), grid, dim3(256), syn_lds<LL_>(DT_), s, p)
#define PV_LOCK_L(LL_)                                   \
    if constexpr (QP) {                                  \
        switch (dt) {                                    \
            case 1: PV_LOCK_DT(LL_, 1); break;           \
            case 2: PV_LOCK_DT(LL_, 2); break;           \
            case 4: PV_LOCK_DT(LL_, 4); break;           \
            default: PV_LOCK_DT(LL_, 0); break;          \
        }                                                \
    } else {                                             \
        PV_LOCK_DT(LL_, 0);                              \
    }
    switch (L) {
        case 128: PV_LOCK_L(128); break;
        case 256: PV_LOCK_L(256); break;
        case 512: PV_LOCK_L(512); break;
        case 1024: PV_LOCK_L(1024); break;
        case 2048: PV_LOCK_DT(2048, 0); break;
        default: return hipErrorInvalidValue;
    }
#undef PV_LOCK_L
#undef PV_LOCK_DT
    return hipGetLastError();
}

hipError_t launch_synthesis_locked(int L, int channels, const SynParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    const int dt = qp ? syn_dt(L, p.hs) : 0;
    return qp ? launch_locked_q<true>(L, dt, grid, p, s) : launch_locked_q<false>(L, dt, grid, p, s);
}

}  // namespace pv
