// pv_resident.hip — the channel-resident STANDARD time stretch: analysis -> unwrap decisions ->
// resynthesis of one channel in ONE workgroup, from its first frame to its last, for the
// configurations whose output phase needs the unwrap count (q > 1; q = 1 has pv_fused.hip).
//
// Why sequential per channel: frame t's output phase needs M(t), the sum of every earlier
// frame's unwrap decision.  The split path cuts a channel into runs, so every
// run's analysis must have finished (k_carry) before any synthesis starts, and each {mag, phase}
// row makes a round trip through HBM (8 KB of the 9.7 KB a frame moves at config 3) although
// no caller sees it (spec = NULL).  Here the rows never leave the CU: a workgroup of three waves
// walks the channel in time,
//   two analysis waves on alternate frames (window, FFT, split, atan2 -> a row in an LDS ring),
//   one synthesis wave that reads the rows in order, makes the decisions inline (as k_rt does),
//   keeps M in registers and runs the register overlap-add (ola_add, ola_shift),
// and the path moves the samples alone: 4 hop + 4 out hop bytes per frame.
//
// Schedule: steps of two frames.  In step j analysis wave a transforms frame 2 j + a into ring
// slot (2 j + a) mod 4 while the synthesis wave consumes frames 2 j - 2 and 2 j - 1 from the
// other two slots; one workgroup barrier ends the step.  Every wave executes
// ceil(frames / 2) + 1 barriers whatever its role and whatever the data, there is no flag, no
// counter and no polling loop, and no workgroup waits for another: the kernel cannot wait
// forever.  Roles are wave-uniform (the wave's index), which with the dispatcher's placement
// gives every SIMD one wave of each role.
//
// An analysis wave's frames are N / 2 samples apart, so in its steady state (frames wholly inside
// the input) it loads only the new half of each frame and rotates the register roles instead of
// moving the old half (ResRot, pv_resident.hpp); the channel's last frames load whole,
// bounds-checked, in a loop of their own.  This translation unit is built without SLP
// vectorisation (-fno-slp-vectorize, Makefile), as pv_analysis.hip is: the per-bin scalar chains
// of the split and the atan2 stay scalar (profiles/resident_ana_c3.txt).
//
// Results are the split path's bit for bit (tests/test_gpu_resident.py,
// tests/test_gpu_resident_tail.py):
//   rows      the pieces k_std_analysis is made of (frame_load_vec / frame_load_checked, win_mul;
//             res_ana_frame: fft_run, bin_l_real, the mirrored-pair split with atan2_pv2 and
//             half_sqrt — pv_frame.hpp, pv_resident.hpp);
//   decisions the contract's one-rounding formula against the previous frame's phase for every
//             frame, phi(-1) = 0 — what k_synthesis does inside a run and k_carry at a run's
//             first frame; the revolution accumulator R = ((p M) mod q) / q is exact, so carrying
//             it across a run boundary equals rebuilding it from the integer carry;
//   seams     the synthesis wave keeps the handle's runs of F frames: at a run boundary the
//             accumulators' tail moves to registers of its own, the accumulators restart at
//             zero, and the next run's first (N - out hop) / out hop frames store head + tail —
//             the sum k_synthesis's epilogue and k_seam make;
//   the end   the last run is virtually padded to F frames (flushes without frames), then its
//             tail goes out, every store checked against the output length.
#include "pv_resident.hpp"

namespace pv {

template <int L, int DT>
__global__ __launch_bounds__(64 * kResWaves, 3) void k_resident(ResidentParams p) {
    using G_ = Geo<L>;
    using RG = ResGeo<L>;
    constexpr int E = G_::E;
    constexpr int N = 2 * L;
    constexpr int NS = E;   // overlap-add slots: positions 128 s + 2 lane + {0, 1}
    constexpr int D = DT;   // slots completed per frame (out hop = 128 DT)
    constexpr int TM = NS - D;  // the overlap, in slots
    static_assert(L <= 512 && 128 * DT < N && TM % D == 0, "register overlap-add, whole frames of overlap");
    extern __shared__ __attribute__((aligned(16))) float2 rsm2[];
    float2* twl = rsm2 + RG::O_TW;
    float2* twsl = rsm2 + RG::O_TWS;
    float2* ring = rsm2 + RG::O_RING;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: SGPR arithmetic
    // role 0, 1: the analysis waves of the even and the odd frames; role 2: the synthesis wave.
    // The role is the wave's index in its workgroup: the dispatcher puts wave w of the r-th
    // workgroup a CU holds on SIMD (w + r) mod 4 (k_fused), so the four
    // workgroups of a CU put their synthesis waves on four different SIMDs and every SIMD holds
    // one wave of each role.  (Rotating the roles with the workgroup index as well undoes that:
    // measured 4.0-4.2 ms per config-3 step against 3.3, profiles/resident_c3.txt.)
    const int role = w;
    float2* tile = rsm2 + RG::O_TILE + w * G_::TILE;
    const int c = blockIdx.x;
    const int frames = p.frames;

    float2 tw0[E];
    load_tw0<L>(tw0, p.tw);
    for (int i = tid; i < L; i += 64 * kResWaves) twl[i] = p.tw[i];
    for (int i = tid; i <= L; i += 64 * kResWaves) twsl[i] = p.tws[i];
    __syncthreads();

    const int nsteps = (frames + 1) / 2 + 1;
    if (role < 2) {
        // ---------------------------------------------------------------- analysis wave
        const float* xc = p.x + (long long)c * p.ldx;
        // frames whose N samples are all inside [0, n) take vector loads (x is aligned: the
        // host's predicate), the last N / hop of a channel the bounds-checked path
        const long long lastfull = (p.n >= N) ? (p.n - N) / p.hop : -1;
        // the wave's frames are t = role + 2 i, i < nmine, one per step; its first nfast are fast
        const int nmine = (frames > role) ? (frames - role + 1) / 2 : 0;
        const long long tl = min(lastfull, (long long)frames - 1);
        const int nfast = (tl >= role) ? (int)((tl - role) / 2) + 1 : 0;
        float2 wv[E];  // the window samples 2 (lane + 64 q) + {0, 1}, for the whole channel
        {
            const float2* w2 = reinterpret_cast<const float2*>(p.win) + lane;
#pragma unroll
            for (int q = 0; q < E; ++q) wv[q] = w2[64 * q];
        }
        using Rot = ResRot<E>;  // the input advances N / 2 samples per frame of a wave (hop = N / 4)
        float2 xr[E];
        // Steady state: a frame of rotation phase r windows its pairs out of the rotated
        // registers, puts the next frame's new pairs (in flight during this frame) into the
        // registers that frees, and transforms.  The prefetch index is clamped: the last fast
        // frame reloads its own pairs, which nothing reads (the frames after it load whole).
        auto fast_frame = [&](auto rc, int i) {
            constexpr int r = decltype(rc)::value, rn = (r + 1) % Rot::RR;
            float2 z[E];
#pragma unroll
            for (int q = 0; q < E; ++q) win_mul(xr[Rot::reg(q, r)], wv[q], z[q]);
            float2 nw[E];
            frame_load_vec<E, E - Rot::D>(xc, (long long)(role + 2 * min(i + 1, nfast - 1)) * p.hop, lane, nw);
#pragma unroll
            for (int q = E - Rot::D; q < E; ++q) xr[Rot::reg(q, rn)] = nw[q];
            res_ana_frame<L>(z, tile, twl, twsl, tw0, lane, ring + ((role + 2 * i) & (kResRing - 1)) * RG::ROW);
            res_barrier();
        };
        int i = 0;
        if (nfast > 0) {
            frame_load_vec<E>(xc, (long long)role * p.hop, lane, xr);
            // one loop of RR frames with an exit after each: it is left at either phase, and
            // holds vector loads only
            for (;;) {
                fast_frame(IC<0>{}, i);
                if (++i == nfast) break;
                fast_frame(IC<1>{}, i);
                if (++i == nfast) break;
            }
        }
        // the channel's last frames (at most N / hop of them, two per wave): whole frames, every
        // sample checked against n — whatever phase the loop above was left at
        for (; i < nmine; ++i) {
            const int t = role + 2 * i;
            frame_load_checked<E>(xc, (long long)t * p.hop, p.n, lane, xr);
            float2 z[E];
#pragma unroll
            for (int q = 0; q < E; ++q) win_mul(xr[q], wv[q], z[q]);
            res_ana_frame<L>(z, tile, twl, twsl, tw0, lane, ring + (t & (kResRing - 1)) * RG::ROW);
            res_barrier();
        }
        // the steps without a frame of this wave (the drain): every wave executes nsteps barriers
        for (; i < nsteps; ++i) res_barrier();
        return;
    }
    // -------------------------------------------------------------------- synthesis wave
    // Two frames of dependent latency per step are the workgroup's critical path (the analysis
    // waves have one frame each and then wait at the barrier), so this wave goes first whenever
    // its SIMD's arbiter has a choice (measured: 3.3 ms per config-3 step against 3.5 without).
    __builtin_amdgcn_s_setprio(3);
    const int hs = p.hs;
    float* outc = p.out + (long long)c * p.ldo;
    float2 gn[NS];  // synthesis gains of the lane's overlap-add slots
    {
        const float2* g2 = reinterpret_cast<const float2*>(p.gain);
#pragma unroll
        for (int s = 0; s < NS; ++s) gn[s] = g2[64 * s + lane];
    }
    // per-lane unwrap constants, as k_synthesis LANEK / RACC: e_k and (p j_k mod q) / q
    float ekr[E + 1];
    unsigned jkr[E + 1];
    {
        const float e_lane = p.ek[lane];
        const unsigned j_lane = __float_as_uint((float)p.jk_mod[lane] * p.inv_q);
        const unsigned j_last = __float_as_uint((float)p.jk_mod[L] * p.inv_q);
#pragma unroll
        for (int i = 0; i <= E; ++i) {
            ekr[i] = e_lane;  // e_L = e_0: lane 0 is the only one that uses bin L
            jkr[i] = (i == E) ? j_last : j_lane;
        }
    }
    const PhaseMap pmap{p.rho * kInv2Pi, p.q, p.p_mod, 1, p.inv_q, (float)p.p_mod * p.inv_q, p.rho < 1.0f ? 1 : 0};
    const SynLds stb{twl, twsl, nullptr, nullptr, nullptr};
    TwReg<E> twr;
#pragma unroll
    for (int q = 0; q < E; ++q) twr.v[q] = lds_ld(&twsl[lane + 64 * q]);

    int M[E + 1];          // R = ((p M) mod q) / q as float bits (synth_frame RACC)
    float phprev[E + 1];   // phi(t - 1); phi(-1) = 0
#pragma unroll
    for (int i = 0; i <= E; ++i) { M[i] = 0; phprev[i] = 0.0f; }
    float2 acc[NS], tail[TM];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int s = 0; s < TM; ++s) tail[s] = make_float2(0.0f, 0.0f);
    int u = 0;           // the frame's index in its run
    int tail_left = 0;   // slots of the previous run's tail not yet added to this run's head

    // positions [t hs, (t + 1) hs) are final: slots 0 .. D-1, plus the previous run's tail
    // where it overlaps (head + tail); CHECKED: past the last frame, against the output length
    // (positions are even and the length is even: a pair is wholly inside or wholly past it)
    auto flush = [&](long long pos, auto checked_tag) {
        constexpr bool CHECKED = decltype(checked_tag)::value;
        f2v v[D];
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = f2v{acc[d].x, acc[d].y};
        if (tail_left > 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = f2v{acc[d].x + tail[d].x, acc[d].y + tail[d].y};
            ola_shift<D>(tail);
            tail_left -= D;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const long long gp = pos + 2 * lane + 128 * d;
            if (!CHECKED || gp + 1 < p.out_len) __builtin_nontemporal_store(v[d], reinterpret_cast<f2v*>(outc + gp));
        }
        ola_shift<D>(acc);
    };

    for (int j = 0; j < nsteps; ++j) {
#pragma unroll 1
        for (int t = 2 * j - 2; t < 2 * j; ++t) {
            if (t < 0 || t >= frames) continue;
            if (u == p.F) {
                // a run ends: its tail waits for the next run's head, the accumulators restart
#pragma unroll
                for (int s = 0; s < TM; ++s) tail[s] = acc[s];
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[s] = make_float2(0.0f, 0.0f);
                tail_left = TM;
                u = 0;
            }
            const float2* row = ring + (t & (kResRing - 1)) * RG::ROW;
            float2 sv[E + 1];
#pragma unroll
            for (int i = 0; i < E; ++i) sv[i] = lds_ld(&row[lane + 64 * i]);
            sv[E] = lds_ld(&row[L]);
            float2 z[E];
            const unsigned tq = ((unsigned)t + 1u) & (p.q - 1u);
            synth_frame<L, 0, false, true, true, true, false, NoHook, TwReg<E>, false, NoEnv>(
                sv, true, tq, M, phprev, pmap, stb, tw0, tile, lane, z, ekr, jkr, NoHook{}, twr, NoEnv{});
            ola_add<L>(z, gn, acc);
            flush((long long)t * hs, std::false_type{});
            ++u;
        }
        res_barrier();
    }
    // the last run's virtual padding to F frames, then its tail
    long long pos = (long long)frames * hs;
    for (; u < p.F && pos < p.out_len; ++u, pos += hs) flush(pos, std::true_type{});
    if (u == p.F) {
#pragma unroll
        for (int s = 0; s < TM; ++s) {
            const long long gp = pos + 2 * lane + 128 * s;
            if (gp + 1 < p.out_len) __builtin_nontemporal_store(f2v{acc[s].x, acc[s].y}, reinterpret_cast<f2v*>(outc + gp));
        }
    }
}

// one round of 1024 channels: four workgroups per CU (160 KB of LDS), three waves per SIMD
static_assert(ResGeo<512>::BYTES <= 40 * 1024, "four workgroups per CU");

bool resident_kernel(int L, int hs) { return L == 512 && hs == 128; }

hipError_t launch_resident(int L, int channels, const ResidentParams& p, hipStream_t s) {
    // (hop = N / 4: the analysis waves' register rotation, ResRot)
    if (!resident_kernel(L, p.hs) || p.hop != L / 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_resident<512, 1>), dim3(channels), dim3(64 * kResWaves), ResGeo<512>::BYTES, s, p);
    return hipGetLastError();
}

}  // namespace pv
