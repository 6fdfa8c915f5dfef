// pv_syn_kernel.hpp — K3 of the split path: the one k_synthesis kernel template (the workgroup
// around syn_run, pv_syn_run.hpp) that every synthesis mode instantiates, and its launch
// geometry.  The translation units pick their modes: pv_kernels.hip MODE 0..3 (with the
// per-lane-constant and partial-row variants), pv_locked.hip kModeLocked, pv_formant.hip
// kModeFormant, pv_warp.hip kModeWarp / kModeLockedWarp, pv_transient.hip kModeReset /
// kModeLockedReset, pv_timemap.hip kModeMap / kModeLockedMap.
#pragma once
#include "pv_syn_run.hpp"

namespace pv {

// ------------------------------------------------------------------ K3 synthesis
// One wave = one run of F frames (virtually padded to F: frames >= `frames` are zero).
// MODE 0/2: STANDARD time stretch / pitch shift — output phase
//         rho*(phi + 2 pi (M_dec + (t+1) j_k)), Hann synthesis window with
//         the overlap normalisation folded into gain[].
// MODE 1: REF_COMPAT — kernel.cu:352-432: x' = m cos(phi), y' = x' sin(phi), C2R N, /N,
//         swap halves (rot = N/2), Hamming window (gain = w/N).
// MODE 3: the pitch shift at ratios >= 1 (at most one source per bin).
// kModeLocked / kModeFormant / kModeWarp / kModeLockedWarp: MODE 0 with identity phase locking
//         (pv_lock.hpp), MODE 2 with the envelope gather (pv_formant.hpp), MODE 0 / kModeLocked
//         with the envelope warp (pv_warp.hpp).  They add no state across frames: the unwrap
//         state, the carries, the run records and the stream segments are the plain modes'.
//         No per-lane-constant (LANEK) or partial-row (NR) variants.
// kModeReset / kModeLockedReset: MODE 0 / kModeLocked with the transient phase reset
//         (pv_transient.hpp): one more additive phase offset per bin, Theta, kept in the wave's
//         registers — from the last flagged run before this one and replaced at the run's own
//         flagged frames (reset_args, pv_kernels.h).
// kModeMap / kModeLockedMap: the time-map stretch (pv_timemap.hpp; out hop = hop): `frames` output
//         frames, each from the two analysis rows around its map position (map_args,
//         pv_kernels.h); the running phase Phi, a 32-bit fraction of a turn, takes the place of
//         the unwrap count in the wave's registers (its carry is k_map_carry's).  Launched with
//         q = 1 (QPOW2): there is no output-phase denominator.  With a map per channel the
//         channel's own row of the map and its own frame count (frames past it are zero).
// Overlap-add: a position is final once the frame that starts after it has been added;
// final samples are stored straight to `out`.
//   DT > 0 (out hop = 128 DT, L <= 1024): in registers.  After the inverse FFT's last pass
//     lane holds points lane + 64 c, i.e. samples 2 lane + {0,1} + 128 c, so every
//     position a lane ever touches is congruent to 2 lane (+1) mod 128: acc[c] covers run
//     positions u*hs + 128 c + 2 lane + {0,1}; per frame the oldest DT slots are stored
//     and the rest shift down.  No LDS ring, no final FFT store.  Runs away from the ends
//     of the output take a loop with unconditional stores and a self-tracked prefetch
//     of the next spectrum row (gload_pairs / vm_wait, pv_device.hpp).
//   DT = 0 (any out hop): per-wave LDS ring of N samples.
// After the loop the three intra-workgroup seams are closed from the neighbours' tails in
// LDS (one barrier); the workgroup's last tail goes to `tails` for k_seam.
// waves per SIMD the synthesis is compiled for (__launch_bounds__): L = 512 at <= 168
// VGPRs; L = 1024 bounded at 1 only so that the compiler may use up to 256 VGPRs: the
// kernels compile to <= 256 without AGPRs, so the 2 waves/SIMD their LDS sets hold
// (tests/test_abi.py checks both)
constexpr int kSynWaves512 = 3;
constexpr int kSynWaves1024 = 1;
// the locked, formant and warp modes (MODE >= kModeLocked) at L = 512: 2 (256 VGPRs).  The
// peak words and the owner search of the locked modes, the envelope row and its prefetch next
// to the spectrum row of the formant and warp modes (the locked warp has all of them) do not
// fit the 168 of kSynWaves512 without spills, which the self-tracked row prefetch of that
// size cannot have (syn_run FASTOK)
constexpr int kSynWaves512Ext = 2;
template <int L, int MODE, int DT, bool QPOW2 = false, bool LANEK = false, int NR = Geo<L>::E>
__global__ __launch_bounds__(256, (L <= 256) ? 4 : (L == 512) ? (MODE >= kModeLocked ? kSynWaves512Ext : kSynWaves512) : (L == 1024) ? kSynWaves1024 : 1) void k_synthesis(SynParams p) {
    using G_ = Geo<L>;
    constexpr bool ROLA = DT > 0;
    constexpr int E = G_::E;
    constexpr int N = 2 * L;
    constexpr int SPW = N / 64;  // samples per lane per frame
    constexpr int B = L + 1;
    constexpr bool GREG = SynTraits<L, MODE, DT, QPOW2>::GREG;  // ROLA gains in registers (else LDS)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2* twl = reinterpret_cast<float2*>(smem);                     // L
    float2* twsl = twl + L;                                            // L (+2 pad)
    float2* tiles = twsl + (L + 2);                                    // 4 x TILE
    float* after_tiles = reinterpret_cast<float*>(tiles + 4 * G_::TILE);
    // 4 x N tails: ROLA writes them only after the frame loop, into the tile area
    // (4 TILE float2 >= 4 N floats); the LDS ring of DT = 0 is live throughout
    float* rings = ROLA ? reinterpret_cast<float*>(tiles) : after_tiles;
    float* gainl = ROLA ? after_tiles : rings + 4 * N;                 // N (unless GREG)
    float* ekl = gainl + (GREG ? 0 : N);                               // B (+pad)
    unsigned* jkl = reinterpret_cast<unsigned*>(ekl + (B + 3));        // B (+pad)
    int* srcl = reinterpret_cast<int*>(jkl + (B + 3));                 // 2 x B (pitch, warp)
    const int hs = p.hs;
    const int TL = N - hs;
    constexpr bool RACC = SynTraits<L, MODE, DT, QPOW2>::RACC;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: SGPR arithmetic
    float2 tw0[Geo<L>::E];
    load_tw0<L>(tw0, p.tw);
    for (int i = tid; i < L; i += 256) { twl[i] = p.tw[i]; twsl[i] = p.tws[i]; }
    if (!GREG)
        for (int i = tid; i < N; i += 256) gainl[i] = p.gain[i];
    if (MODE != 1 && !mode_is_map(MODE)) {  // (the map modes read no unwrap table)
        for (int i = tid; i < B; i += 256) {
            ekl[i] = p.ek[i];
            // RACC: (p j_k mod q) / q as a float (exact: q <= 4096)
            jkl[i] = RACC ? __float_as_uint((float)p.jk_mod[i] * p.inv_q) : p.jk_mod[i];
            // the pitch map {first source, count}; the warp map {i_k, bits of f_k} travels in
            // the pitch map's fields (a time stretch has no bin map).  kModeLocked: nothing
            if (MODE == 2 || MODE == kModeFormant || mode_is_warp(MODE)) {
                srcl[2 * i] = p.src_first[i];
                srcl[2 * i + 1] = p.src_cnt[i];
            }
            // MODE 3: the source's byte offset in a wave's tile, L + 1 (zero slot) if none
            if (MODE == 3) srcl[i] = (int)sizeof(float2) * (p.src_first[i] >= 0 ? p.src_first[i] : L + 1);
        }
    }
    float* ring = rings + w * N;  // ROLA: the run's tail, written after the frame loop
    if (!ROLA) {
#pragma unroll
        for (int i = 0; i < SPW; ++i) ring[lane + 64 * i] = 0.0f;
    }
    __syncthreads();

    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    const int t0 = run * p.F;
    int frames_c = p.frames;
    if constexpr (mode_is_map(MODE)) {  // a map per channel may end before `frames` (map_args, pv_kernels.h)
        const int* counts = map_args(p).counts;
        if (counts) frames_c = __builtin_amdgcn_readfirstlane(counts[c]);
    }
    const int nfr = max(0, min(p.F, frames_c - t0));  // real frames of this wave's run
    float* outc = p.out + (long long)c * p.ldo;
    const long long obase = (long long)t0 * hs;

    int M[E + 1];
    float phprev[E + 1];
    if (MODE != 1 && nfr > 0) {
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
    constexpr int NS = SynTraits<L, MODE, DT, QPOW2>::NS, D = SynTraits<L, MODE, DT, QPOW2>::D;
    float2 acc[NS];
    if constexpr (mode_is_reset(MODE)) {
        // Theta of the last flagged run before this one (k_reset wrote it), or 0; the run's own
        // flagged frames replace it as the wave meets them
        float th[E + 1];
        int prr = -1;
        const ResetArgs ra = reset_args(p);
        if (nfr > 0) prr = __builtin_amdgcn_readfirstlane(ra.prev_reset_run[(long long)c * p.nruns + run]);
        const float* ths = ra.theta + ((long long)c * p.nruns + (prr >= 0 ? prr : 0)) * p.bins_pad;
#pragma unroll
        for (int i = 0; i <= E; ++i) th[i] = 0.0f;
        if (prr >= 0) { PV_FOR_BINS(E, lane, { th[i] = ths[k]; }) }
        const ResetRun<E> rs{th, ra.flags + (long long)c * ra.ld_flags + t0};
        syn_run<L, MODE, DT, QPOW2, LANEK, NR, ResetRun<E>>(
            p, SynCarve{twl, twsl, tiles, rings, gainl, ekl, jkl, srcl}, tw0, lane, w, c, t0, nfr, M, phprev, acc, rs);
    } else if constexpr (mode_is_map(MODE)) {
        // M holds Phi at the run's first frame: the carry k_map_carry wrote (loaded above)
        const MapArgs ma = map_args(p);
        syn_run<L, MODE, DT, QPOW2, LANEK, NR, NoResetRun, MapRun>(
            p, SynCarve{twl, twsl, tiles, rings, gainl, ekl, jkl, srcl}, tw0, lane, w, c, t0, nfr, M, phprev, acc,
            NoResetRun{}, MapRun{ma.map + (long long)c * ma.ld_map + t0, ma.aframes});
    } else
    syn_run<L, MODE, DT, QPOW2, LANEK, NR>(
        p, SynCarve{twl, twsl, tiles, rings, gainl, ekl, jkl, srcl}, tw0, lane, w, c, t0, nfr, M, phprev, acc);
    if constexpr (ROLA) {
        // the run's tail (positions F*hs + j, j < N - hs) -> ring[j], over the tiles
        __syncthreads();
        float2* r2 = reinterpret_cast<float2*>(ring);
#pragma unroll
        for (int s = 0; s < NS - D; ++s) r2[64 * s + lane] = acc[s];
    }
    __syncthreads();
    const int nwg = (p.nruns + 3) / 4;
    const bool last = (blockIdx.x + 1 >= nwg);
    // the 8-byte seam epilogue below: MODE 0..3.  The locked, formant and warp modes take the
    // per-sample path only because they always have; enabling it there is a measured change
    // of its own
    constexpr bool ALIGNED_SEAMS = MODE <= 3;
    if constexpr (ALIGNED_SEAMS && ROLA && N > 128 * DT) {
        if (p.out_aligned) {
            // the overlap is TM = (N - 128 DT) / 128 float2 per lane at positions 2 lane +
            // 128 m; positions are even and out_len is even, so a pair is wholly inside out
            // or wholly past it.  The head read-back is one batch of loads and one wait (per
            // 64 samples, a load-add-store was one serialized round trip: 14 at config 3)
            constexpr int TM = (N - 128 * DT) / 128;
            const float2* own2 = reinterpret_cast<const float2*>(ring) + lane;
            if (w > 0) {
                const float2* prev2 = reinterpret_cast<const float2*>(rings + (w - 1) * N) + lane;
                f2v hd[TM];
#pragma unroll
                for (int m = 0; m < TM; ++m) {
                    const long long gp = obase + 2 * lane + 128 * m;
                    hd[m] = (gp < p.out_len) ? *reinterpret_cast<const f2v*>(outc + gp) : f2v{0.0f, 0.0f};
                }
#pragma unroll
                for (int m = 0; m < TM; ++m) {
                    const long long gp = obase + 2 * lane + 128 * m;
                    const float2 t = prev2[64 * m];
                    if (gp < p.out_len)
                        __builtin_nontemporal_store(f2v{hd[m].x + t.x, hd[m].y + t.y}, reinterpret_cast<f2v*>(outc + gp));
                }
            }
            if (w == 3) {
                const long long nb = obase + (long long)p.F * hs + 2 * lane;
                float* tdst = p.tails + ((long long)c * nwg + blockIdx.x) * p.tail_len + 2 * lane;
#pragma unroll
                for (int m = 0; m < TM; ++m) {
                    const float2 v = own2[64 * m];
                    if (last) {
                        if (nb + 128 * m < p.out_len)
                            __builtin_nontemporal_store(f2v{v.x, v.y}, reinterpret_cast<f2v*>(outc + nb + 128 * m));
                    } else {
                        *reinterpret_cast<f2v*>(tdst + 128 * m) = f2v{v.x, v.y};
                    }
                }
            }
            return;
        }
    }
    // seams: run w's tail (positions F*hs + j) overlaps run w+1's head, which that run has
    // stored; every access is bounds-checked against out_len
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

// ------------------------------------------------------------------ launch geometry (host)
template <int L>
inline size_t syn_lds(int dt) {
    const int ring_floats = (dt > 0) ? 0 : 4 * 2 * L;               // ROLA: tails alias the tiles
    const int gain_floats = syn_gains_in_regs(L, dt) ? 0 : 2 * L;
    return sizeof(float2) * (L + (L + 2) + 4 * Geo<L>::TILE) +
           sizeof(float) * (ring_floats + gain_floats) + sizeof(float) * 4 * (L + 1 + 3);
}

// register overlap-add slots per frame (out hop = 128 DT), 0 = LDS ring
inline int syn_dt(int L, int hs) {
    if (L > 1024 || hs % 128 != 0) return 0;
    const int d = hs / 128;
    return (d == 1 || d == 2 || d == 4) ? d : 0;
}

// The launch of a mode without LANEK / NR variants (locked, formant, warp), the kernel of
// launch_synthesis's plain modes for the same geometry: register overlap-add (out hop 128, 256
// or 512, L <= 1024) where q is a power of two <= 4096 (QP), the LDS ring otherwise.
// L = 128 .. MAXL; above 1024 only the LDS ring exists.
template <int L, int MODE, bool QP>
inline void launch_syn_plain_l(int dt, dim3 grid, const SynParams& p, hipStream_t s) {
    if constexpr (QP && L <= 1024) {
        switch (dt) {
            case 1: hipLaunchKernelGGL((k_synthesis<L, MODE, 1, QP>), grid, dim3(256), syn_lds<L>(1), s, p); return;
            case 2: hipLaunchKernelGGL((k_synthesis<L, MODE, 2, QP>), grid, dim3(256), syn_lds<L>(2), s, p); return;
            case 4: hipLaunchKernelGGL((k_synthesis<L, MODE, 4, QP>), grid, dim3(256), syn_lds<L>(4), s, p); return;
        }
    }
    hipLaunchKernelGGL((k_synthesis<L, MODE, 0, QP>), grid, dim3(256), syn_lds<L>(0), s, p);
}

template <int MODE, bool QP, int MAXL>
inline hipError_t launch_syn_plain(int L, int dt, dim3 grid, const SynParams& p, hipStream_t s) {
    static_assert(MAXL == 1024 || MAXL == 2048, "the sizes a mode is built for end at 1024 or 2048");
    switch (L) {
        case 128: launch_syn_plain_l<128, MODE, QP>(dt, grid, p, s); break;
        case 256: launch_syn_plain_l<256, MODE, QP>(dt, grid, p, s); break;
        case 512: launch_syn_plain_l<512, MODE, QP>(dt, grid, p, s); break;
        case 1024: launch_syn_plain_l<1024, MODE, QP>(dt, grid, p, s); break;
        default:
            if constexpr (MAXL == 2048) {
                if (L == 2048) { launch_syn_plain_l<2048, MODE, QP>(dt, grid, p, s); break; }
            }
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pv
