// pv_transient.hip — transient phase reset of the STANDARD time stretch (pv_set_transient;
// DESIGN.md §3.11): the onset detector (k_onset, k_pick), the reset offsets of the flagged runs
// (k_reset) and the instantiations of k_synthesis (pv_syn_kernel.hpp) in the reset modes.
//
//   k_onset   {rise, tot} of every frame from the analysis rows' magnitudes
//   k_pick    flags = local maxima of rise among the frames with rise > thr tot, and for every
//             run the last run before it that holds a flagged frame
//   k_reset   Theta after the last flagged frame of every run that holds one, from the run's
//             carry and its rows: the decisions k_synthesis makes, made again
//   k_synthesis<kModeReset / kModeLockedReset>   MODE 0 / kModeLocked with Theta in registers
// Nothing waits on another workgroup, nothing allocates or synchronises: all capturable.
//
// A translation unit of its own: the kernels compile next to the other modes', and their
// registers are checked file by file (tests/test_transient_ref.py).
#include "pv_syn_kernel.hpp"

namespace pv {

// ------------------------------------------------------------------ k_onset
// One wave = one run of F frames, 4 runs per workgroup.  The lane holds the magnitudes of bins
// lane + 64 i (i < E) and lane 0 that of bin L (slot E; 0 on the other lanes, which adds
// nothing).  The next row is loaded before the current one is summed; the previous row's
// magnitudes stay in registers (a run's first frame reads row t0 - 1 once).  Per-lane partial
// sums in slot order, then a butterfly over the lanes (xor 32, 16, .. 1): a fixed order.
// maxNum: a NaN magnitude adds 0 to both sums.
template <int L>
__global__ __launch_bounds__(256) void k_onset(OnsetParams p) {
    constexpr int E = L / 64;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    if (run >= p.nruns) return;
    const int t0 = run * p.F;
    const int nfr = min(p.F, p.frames - t0);
    const float2* specc = p.spec + (long long)c * p.ld_spec;
    const bool packed = p.packed != 0;
    // PV_SPEC_PACKED rows: bins 0 and L are the sign-coded magnitudes of slot 0
    auto load = [&](int t, float (&m)[E + 1]) {
        const float2* row = specc + (long long)t * p.spec_stride;
#pragma unroll
        for (int i = 0; i < E; ++i) m[i] = row[lane + 64 * i].x;
        const float2 last = row[packed ? 0 : L];  // one address on every lane
        if (packed && lane == 0) m[0] = __builtin_fabsf(m[0]);
        m[E] = (lane == 0) ? (packed ? __builtin_fabsf(last.y) : last.x) : 0.0f;
    };
    float prev[E + 1], cur[E + 1];
    if (t0 > 0) {
        load(t0 - 1, prev);
    } else {
#pragma unroll
        for (int i = 0; i <= E; ++i) prev[i] = 0.0f;
    }
    load(t0, cur);
    for (int u = 0; u < nfr; ++u) {
        float nxt[E + 1];
        load(t0 + min(u + 1, nfr - 1), nxt);  // (the run's last frame re-reads its own row)
        float rise = 0.0f, tot = 0.0f;
#pragma unroll
        for (int i = 0; i <= E; ++i) {
            rise += __builtin_fmaxf(cur[i] - prev[i], 0.0f);
            tot += __builtin_fmaxf(cur[i], 0.0f);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            rise += __shfl_xor(rise, d);
            tot += __shfl_xor(tot, d);
        }
        if (lane == 0) p.dst[(long long)c * p.ld_dst + t0 + u] = make_float2(rise, tot);
#pragma unroll
        for (int i = 0; i <= E; ++i) {
            prev[i] = cur[i];
            cur[i] = nxt[i];
        }
    }
}

// ------------------------------------------------------------------ k_pick
// One workgroup per channel.  With strengths: every thread decides the flags of frames tid,
// tid + 256, ..; then wave 0 scans the runs 64 at a time: a lane looks for a flag byte in its
// run, the ballot of the lanes that found one gives every lane the nearest flagged run below it
// (find-last-bit of the word masked below the lane), or the last one of the earlier words.
__global__ __launch_bounds__(256) void k_pick(PickParams p) {
    const int c = blockIdx.x;
    unsigned char* fl = p.flags + (long long)c * p.ld_flags;
    if (p.strength) {
        const float2* s = p.strength + (long long)c * p.ld_strength;
        for (int t = threadIdx.x; t < p.frames; t += 256) {
            const float2 v = s[t];
            const float before = (t > 0) ? s[t - 1].x : 0.0f;
            const float after = (t + 1 < p.frames) ? s[t + 1].x : 0.0f;
            const bool f = t >= 1 && v.x > p.thr * v.y && v.x > before && v.x >= after;
            fl[t] = f ? 1 : 0;
        }
        __syncthreads();
    }
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    int last = -1;  // wave-uniform: the last flagged run of the words before this one
    for (int base = 0; base < p.nruns; base += 64) {
        const int r = base + lane;
        bool has = false;
        if (r < p.nruns) {
            const int t0 = r * p.F, t1 = min(t0 + p.F, p.frames);
            for (int t = t0; t < t1; ++t) has = has || fl[t] != 0;
        }
        const unsigned long long word = __builtin_amdgcn_ballot_w64(has);
        const unsigned long long below = word & ((1ull << lane) - 1ull);
        if (r < p.nruns)
            p.prev_reset_run[(long long)c * p.nruns + r] = below ? base + 63 - __builtin_clzll(below) : last;
        if (word) last = base + 63 - __builtin_clzll(word);
    }
}

// ------------------------------------------------------------------ k_reset
// One wave per (channel, run), 4 runs per workgroup; a run without a flagged frame exits.  The
// wave loads the run's carry (the unwrap count at the run's first frame, that frame's decision
// included: k_synthesis's convention) and walks the rows up to the run's last flagged frame with
// k_synthesis's decisions (unwrap_count), then forms that frame's locked-form phase with
// synth_frame's operations — the revolution form for power-of-two q <= 4096 (QPOW2; exact, so
// R equals synth_frame's accumulator bit for bit), the integer forms otherwise — and writes
// Theta.  q = 1: no carry, no walk (the count drops out of the output phase).
template <int L, bool QPOW2>
__global__ __launch_bounds__(256) void k_reset(ResetParams p) {
    constexpr int E = L / 64;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    if (run >= p.nruns) return;
    const int t0 = run * p.F;
    const int nfr = min(p.F, p.frames - t0);
    const unsigned char* fl = p.flags + (long long)c * p.ld_flags + t0;
    int ulast = -1;  // the run's last flagged frame (wave-uniform)
    for (int b = 0; b < nfr; b += 64) {
        const int uu = b + lane;
        const unsigned long long word = __builtin_amdgcn_ballot_w64(uu < nfr && fl[uu < nfr ? uu : 0] != 0);
        if (word) ulast = b + 63 - __builtin_clzll(word);
    }
    if (ulast < 0) return;
    const float2* specc = p.spec + (long long)c * p.ld_spec;
    const bool packed = p.packed != 0;
    auto load = [&](int t, float (&ph)[E + 1]) {
        const float2* row = specc + (long long)t * p.spec_stride;
        float2 sv[E + 1];
        PV_FOR_BINS(E, lane, {
            if (i < E || !packed) sv[i] = row[k];
        })
        if (packed && lane == 0) unpack_real_bins(sv[0], sv[0], sv[E]);
        PV_FOR_BINS(E, lane, { ph[i] = sv[i].y; })
    };
    const bool walk = p.carry != nullptr;
    const int* cr = walk ? p.carry + ((long long)c * p.nruns + run) * p.bins_pad : nullptr;
    int M[E + 1];
    float ek[E + 1], ph[E + 1];
    unsigned jk[E + 1];
    PV_FOR_BINS(E, lane, {
        M[i] = walk ? cr[k] : 0;
        ek[i] = p.ek[k];
        jk[i] = p.jk_mod[k];
    })
    load(walk ? t0 : t0 + ulast, ph);
    if (walk) {
        for (int u = 1; u <= ulast; ++u) {
            float pn[E + 1];
            load(t0 + u, pn);
            PV_FOR_BINS(E, lane, {
                M[i] += unwrap_count(pn[i], ph[i], ek[i]);
                ph[i] = pn[i];
            })
        }
    }
    const unsigned q32 = (unsigned)p.q, pmod = (unsigned)p.p_mod;
    const unsigned t1 = (unsigned)(t0 + ulast + 1);
    const float rrl = p.rho * kInv2Pi - kInv2Pi;
    float* dst = p.theta + ((long long)c * p.nruns + run) * p.bins_pad;
    if constexpr (QPOW2) {
        const unsigned qm = q32 - 1u;
        const float tqf = (float)(t1 & qm);
        PV_FOR_BINS(E, lane, {
            const float R = (float)((pmod * ((unsigned)M[i] & qm)) & qm) * p.inv_q;
            const float tj = __builtin_amdgcn_fractf(tqf * ((float)jk[i] * p.inv_q));
            dst[k] = reset_offset(__builtin_fmaf(rrl, ph[i], R + tj));
        })
    } else if (p.q_pow2) {
        const unsigned qm = q32 - 1u;
        const unsigned tq = t1 & qm;
        PV_FOR_BINS(E, lane, {
            const unsigned x = pmod * ((unsigned)M[i] & qm) + tq * jk[i];
            dst[k] = reset_offset(__builtin_fmaf(rrl, ph[i], (float)(x & qm) * p.inv_q));
        })
    } else {
        const unsigned tq = t1 % q32;
        PV_FOR_BINS(E, lane, {
            int mdq = M[i] % (int)q32;
            mdq += (mdq < 0) ? (int)q32 : 0;
            const unsigned x = pmod * (unsigned)mdq + tq * jk[i];
            dst[k] = reset_offset(__builtin_fmaf(rrl, ph[i], (float)(x % q32) * p.inv_q));
        })
    }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_onset(int L, int channels, const OnsetParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    switch (L) {
        case 128: hipLaunchKernelGGL(k_onset<128>, grid, dim3(256), 0, s, p); break;
        case 256: hipLaunchKernelGGL(k_onset<256>, grid, dim3(256), 0, s, p); break;
        case 512: hipLaunchKernelGGL(k_onset<512>, grid, dim3(256), 0, s, p); break;
        case 1024: hipLaunchKernelGGL(k_onset<1024>, grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_pick(int channels, const PickParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_pick, dim3(channels), dim3(256), 0, s, p);
    return hipGetLastError();
}

template <bool QP>
static hipError_t launch_reset_q(int L, dim3 grid, const ResetParams& p, hipStream_t s) {
    switch (L) {
        case 128: hipLaunchKernelGGL((k_reset<128, QP>), grid, dim3(256), 0, s, p); break;
        case 256: hipLaunchKernelGGL((k_reset<256, QP>), grid, dim3(256), 0, s, p); break;
        case 512: hipLaunchKernelGGL((k_reset<512, QP>), grid, dim3(256), 0, s, p); break;
        case 1024: hipLaunchKernelGGL((k_reset<1024, QP>), grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// (QPOW2 exactly where launch_synthesis_reset takes the QPOW2 synthesis)
hipError_t launch_reset(int L, int channels, const ResetParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    return qp ? launch_reset_q<true>(L, grid, p, s) : launch_reset_q<false>(L, grid, p, s);
}

// the kernel of launch_synthesis_locked for the same geometry (launch_syn_plain), up to L = 1024
hipError_t launch_synthesis_reset(int L, int lock, int channels, const SynParams& p, hipStream_t s) {
    const ResetArgs ra = reset_args(p);
    if (!ra.flags || !ra.theta || !ra.prev_reset_run) return hipErrorInvalidValue;
    dim3 grid((p.nruns + 3) / 4, channels);
    const bool qp = p.q_pow2 && p.q <= 4096ull;
    const int dt = qp ? syn_dt(L, p.hs) : 0;
    if (lock) return qp ? launch_syn_plain<kModeLockedReset, true, 1024>(L, dt, grid, p, s)
                        : launch_syn_plain<kModeLockedReset, false, 1024>(L, dt, grid, p, s);
    return qp ? launch_syn_plain<kModeReset, true, 1024>(L, dt, grid, p, s)
              : launch_syn_plain<kModeReset, false, 1024>(L, dt, grid, p, s);
}

}  // namespace pv
