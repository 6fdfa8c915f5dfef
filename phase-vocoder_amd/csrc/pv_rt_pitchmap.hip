// pv_rt_pitchmap.hip — the real-time pitch map (pv_rt_pitchmap_push): the
// streaming form of "time map, then variable-rate resampling" (pv_pitchmap_process, §3.12 / §3.13),
// one fp32 pitch ratio per pushed frame, read from memory when the launch runs.  Two launches per
// callback:
//
//   k_rt_map          a wave per channel, as k_rt (pv_rt.hip): the same analysis of the pushed
//                     frame (pv_frame.hpp: the row's phases are the oracle's bit for bit), then the
//                     span from the previous row to this one.  Its step d = (int64)(r' 2^32) is the
//                     frame's clamped ratio, its length hop d; the stretched frames v with
//                     Sigma_b <= v hop 2^32 < Sigma_{b+1} (0 to 4 of them, wave-uniform) are built by
//                     synth_frame in the map modes from the two rows — magnitude lerp at
//                     a = (float)(off / (hop d)) (one fp64 division of exact integers), Phi advanced
//                     by P(b+1) - P(b) after each — overlap-added at the hop, and each appends the
//                     hop samples it completes to the channel's scratch row.  The step goes into the
//                     channel's ring.  The two rows live in LDS ({mag, bits of P}, swapped by a
//                     wave-uniform index), Phi in registers; between launches the previous row, Phi,
//                     the input history, the overlap accumulator and RtMapState are in HBM.
//   k_rt_varresample  a workgroup per channel, as k_rt_resample (pv_rt_pitch.hip).  Output block
//                     t - 1 - G of pushed frame t (zeros below block 0) takes the oldest step of
//                     the ring: Sq_b and W_b in fp64 from d_b (pvtab::var_block_filter's
//                     operations), the outputs at rpos + j d_b into the row, every tap computed by
//                     pv_varresample.hpp's code, one thread per output and the taps in rising
//                     order — the accumulation order depends on the tap index alone, so the stream
//                     does not depend on how it is cut into pushes.  Then the samples no later
//                     block reads leave the row: the rest moves to its front, 256 samples at a
//                     time through registers with a barrier between a chunk's reads and its writes
//                     (the move goes down, so a chunk's writes stay below every later read).
//
// G (pvtab::rt_pitchmap_plan) is the number of callbacks an output block waits so that every
// stretched sample it reads is final; the row and the ring are sized by the host from G, the ratio
// range and the largest push.  Every position is relative to the row, every counter saturates: the
// stream can run for ever.
//
// A kernel file of its own, so every other kernel keeps its code.
#include "pv_frame.hpp"
#include "pv_kernels.h"
#include "pv_varresample.hpp"

namespace pv {

// k_rt's carve-up (pv_rt.hip RtGeo) without the unwrap and pitch tables, plus two spectrum rows
// per wave
template <int L>
struct RtMapGeo {
    static constexpr int N = 2 * L;
    static constexpr int B = L + 1;
    static constexpr int W = (L <= 512) ? 4 : 2;
    static constexpr int TILE = Geo<L>::TILE;
    static constexpr int RB = B + 1;                        // float2 slots of a row (even)
    // float offsets
    static constexpr int O_TW = 0;                          // L float2
    static constexpr int O_TWS = O_TW + 2 * L;              // L+1 float2 (+1 pad)
    static constexpr int O_TILE = O_TWS + 2 * (L + 2);      // W x TILE float2
    static constexpr int O_WIN = O_TILE + 2 * W * TILE;     // N
    static constexpr int O_GAIN = O_WIN + N;                // N
    static constexpr int O_BUF = O_GAIN + N;                // W x N input window
    static constexpr int O_OLA = O_BUF + W * N;             // W x N overlap accumulator
    static constexpr int O_ROWS = O_OLA + W * N;            // W x 2 x RB float2 {mag, bits of P}
    static_assert(O_TILE % 2 == 0 && O_ROWS % 2 == 0, "float2 regions are 8-byte aligned");
    static constexpr int FLOATS = O_ROWS + W * 2 * 2 * RB;
    static constexpr size_t BYTES = sizeof(float) * FLOATS;
};

namespace {
// a wave-uniform 64-bit value, kept in scalar registers
__device__ __forceinline__ long long uniform64(long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
}  // namespace

template <int L, bool LOCKED>
__global__ __launch_bounds__(256) void k_rt_map(RtMapParams pp) {
    using G_ = Geo<L>;
    using R_ = RtMapGeo<L>;
    constexpr int MODE = LOCKED ? kModeLockedMap : kModeMap;
    constexpr int E = G_::E;
    constexpr int N = R_::N;
    constexpr int B = R_::B;
    constexpr int W = R_::W;
    constexpr int SPW = N / 64;
    static_assert(!LOCKED || 2 * R_::TILE >= L + 2, "theta scratch of the locked step: L + 2 floats");
    const RtParams& p = pp.rt;
    extern __shared__ __attribute__((aligned(16))) float rsm[];
    float2* twl = reinterpret_cast<float2*>(rsm + R_::O_TW);
    float2* twsl = reinterpret_cast<float2*>(rsm + R_::O_TWS);
    float* winl = rsm + R_::O_WIN;
    float* gainl = rsm + R_::O_GAIN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: SGPR arithmetic
    float2 tw0[E];
    load_tw0<L>(tw0, p.tw);
    for (int i = tid; i < L; i += 64 * W) twl[i] = p.tw[i];
    for (int i = tid; i < B; i += 64 * W) twsl[i] = p.tws[i];
    for (int i = tid; i < N; i += 64 * W) { winl[i] = p.win[i]; gainl[i] = p.gain[i]; }
    __syncthreads();

    const int c = blockIdx.x * W + w;
    if (c >= p.channels) return;
    float2* tile = reinterpret_cast<float2*>(rsm + R_::O_TILE) + w * R_::TILE;
    float* buf = rsm + R_::O_BUF + w * N;
    float* olab = rsm + R_::O_OLA + w * N;
    float2* rows = reinterpret_cast<float2*>(rsm + R_::O_ROWS) + w * 2 * R_::RB;
    const int hop = p.hop;
    const int keep = N - hop;  // history samples carried to the next frame, and overlap samples

    float* hist = p.hist + (long long)c * N;
    float* olag = p.ola + (long long)c * N;
    for (int j = lane; j < keep; j += 64) buf[j] = hist[j];
    for (int j = lane; j < N; j += 64) olab[j] = (j < keep) ? olag[j] : 0.0f;
    int M[E + 1];          // Phi, a 32-bit fraction of a turn per bin (synth_frame's map modes)
    float unused[E + 1];   // (the map modes keep no unwrap state)
    float2* prevg = pp.prev + (long long)c * p.bins_pad;
    {
        const unsigned* Fg = pp.phi + (long long)c * p.bins_pad;
        PV_FOR_BINS(E, lane, { M[i] = (int)Fg[k]; unused[i] = 0.0f; rows[k] = prevg[k]; })
    }
    int cur = 0;  // the half of `rows` that holds the previous row (wave-uniform)
    const RtMapState st = pp.st[c];
    long long off = uniform64(st.off);
    int fill = __builtin_amdgcn_readfirstlane(st.fill);
    int nsteps = __builtin_amdgcn_readfirstlane(st.nsteps);
    int have = __builtin_amdgcn_readfirstlane(st.rows);
    long long* ringc = pp.ring + (long long)c * pp.ring_cap;
    float* rowg = pp.row + (long long)c * pp.ld_row + pp.K;
    const long long unit = (long long)hop << 32;  // a stretched frame's hop, 2^-32 samples
    const PhaseMap pmap{};
    const SynLds stb{twl, twsl, nullptr, nullptr, nullptr};
    const float* inc = p.in + (long long)c * p.ldi;

    for (int f = 0; f < p.nframes; ++f) {
        for (int j = lane; j < hop; j += 64) buf[keep + j] = inc[(long long)f * hop + j];
        wave_lds_sync();
        // ---- analysis (k_rt's: the same operations as k_std_analysis)
        float2 z[E];
        {
            const float2* b2 = reinterpret_cast<const float2*>(buf) + lane;
            const float2* w2 = reinterpret_cast<const float2*>(winl) + lane;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const float2 xv = lds_ld(&b2[64 * q]);
                const float2 wv = lds_ld(&w2[64 * q]);
                win_mul(xv, wv, z[q]);
            }
        }
        fft_run<L, false, false>(z, tile, twl, tw0, lane);  // the split reads the last pass's registers
        float2* rp = rows + cur * R_::RB;        // row b
        float2* rn = rows + (cur ^ 1) * R_::RB;  // row b + 1, analysed now
        float2* srow = (p.spec != nullptr)
                           ? p.spec + (long long)c * p.ld_spec + (long long)f * p.spec_stride
                           : nullptr;
        constexpr int CH = 3;
        static_for<0, (E + CH) / CH>([&](auto ic) {
            constexpr int i0 = decltype(ic)::value * CH;
            float2 X[CH];
            split_chunk_bp<L, CH, false, i0>(z, twsl, lane, X);
#pragma unroll
            for (int c2 = 0; c2 < CH; ++c2) {
                const int i = i0 + c2;
                if (i > E) break;
                const float ph = atan2_pv(X[c2].y, X[c2].x);
                const float mag = __builtin_amdgcn_sqrtf(__builtin_fmaf(X[c2].x, X[c2].x, X[c2].y * X[c2].y));
                if (i < E || lane == 0) {
                    const int k = (i == E) ? L : lane + 64 * i;
                    if (srow != nullptr) srow[k] = make_float2(mag, ph);
                    rn[k] = make_float2(mag, __uint_as_float(phase_turns(ph)));
                }
            }
        });
        wave_lds_sync();
        // ---- the frame's step: clamped with minNum / maxNum (a NaN reads as ratio_min)
        const float rq = pp.ratio ? pp.ratio[(long long)c * pp.ldr + f] : 1.0f;
        const float rv = (rq == rq) ? rq : pp.ratio_min;  // (a signalling NaN too)
        const float rc = __builtin_fminf(__builtin_fmaxf(rv, pp.ratio_min), pp.ratio_max);
        const long long d = uniform64((long long)(rc * 0x1p32f));
        if (have == 0) {
            // the stream's first row: Phi(0) = P(0); its ratio is read and ignored
            PV_FOR_BINS(E, lane, { M[i] = (int)__float_as_uint(lds_ld(&rn[k]).y); })
            have = 1;
            off = 0;
        } else {
            const long long span = (long long)hop * d;  // Sigma_{b+1} - Sigma_b
            while (off < span) {
                // ---- one stretched frame at row b + a (DESIGN.md §3.12 with i_u = b)
                const float a = (float)((double)off / (double)span);
                float2 sv[E + 1];
                PV_FOR_BINS(E, lane, {
                    const float2 r0 = lds_ld(&rp[k]);
                    const float m1 = lds_ld(&rn[k]).x;
                    sv[i] = make_float2(__builtin_fmaf(a, m1 - r0.x, r0.x), r0.y);
                })
                float ekr[E + 1];       // unused (KREG = false)
                unsigned jkr[E + 1];
                synth_frame<L, MODE, true, true>(sv, true, 0u, M, unused, pmap, stb, tw0, tile, lane, z, ekr, jkr);
                // ---- overlap-add at the hop, append the hop samples the frame completes, shift
                const float* ty = reinterpret_cast<const float*>(tile);
                float nv[SPW];
#pragma unroll
                for (int i = 0; i < SPW; ++i) {
                    const int n = lane + 64 * i;
                    const float yv = ty[2 * G_::pad(n >> 1) + (n & 1)];
                    olab[n] = __builtin_fmaf(yv, gainl[n], olab[n]);
                }
                wave_lds_sync();
                for (int j = lane; j < hop; j += 64) rowg[fill + j] = olab[j];  // (in the row: the host's sizing)
                fill += hop;
#pragma unroll
                for (int i = 0; i < SPW; ++i) {
                    const int n = lane + 64 * i;
                    nv[i] = (n < keep) ? olab[n + hop] : 0.0f;
                }
                wave_lds_sync();
#pragma unroll
                for (int i = 0; i < SPW; ++i) olab[lane + 64 * i] = nv[i];
                wave_lds_sync();
                // Phi += P(b + 1) - P(b), modulo 2^32
                PV_FOR_BINS(E, lane, {
                    M[i] = (int)((unsigned)M[i] + (__float_as_uint(lds_ld(&rn[k]).y) - __float_as_uint(lds_ld(&rp[k]).y)));
                })
                off += unit;
            }
            off -= span;
            if (lane == 0) ringc[nsteps] = d;  // (nsteps < ring_cap: at most G wait between callbacks)
            ++nsteps;
        }
        cur ^= 1;
        // input window moves by one hop
        float nv[SPW];
#pragma unroll
        for (int i = 0; i < SPW; ++i) {
            const int n = lane + 64 * i;
            nv[i] = (n < keep) ? buf[n + hop] : 0.0f;
        }
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < SPW; ++i) {
            const int n = lane + 64 * i;
            if (n < keep) buf[n] = nv[i];
        }
        wave_lds_sync();
    }
    // ---- state back to HBM
    for (int j = lane; j < keep; j += 64) { hist[j] = buf[j]; olag[j] = olab[j]; }
    {
        unsigned* Fg = pp.phi + (long long)c * p.bins_pad;
        const float2* rl = rows + cur * R_::RB;
        PV_FOR_BINS(E, lane, { Fg[k] = (unsigned)M[i]; prevg[k] = lds_ld(&rl[k]); })
    }
    if (lane == 0) {  // (rpos and emitted are k_rt_varresample's)
        RtMapState* sg = pp.st + c;
        sg->off = off;
        sg->rows = have;
        sg->fill = fill;
        sg->nsteps = nsteps;
    }
}

// a[j] = a[j + delta], j < n, delta > 0: by the whole workgroup, 256 elements at a time through
// registers.  A chunk's writes [j0, j0 + 256) lie below the reads of every later chunk
// (>= j0 + 256 + delta), so one barrier per chunk, between its reads and its writes, orders all.
template <typename T>
__device__ __forceinline__ void move_down(T* a, int n, int delta, int tid) {
    for (int j0 = 0; j0 < n; j0 += 256) {  // (uniform bound: every thread reaches the barrier)
        const int j = j0 + tid;
        T v{};
        if (j < n) v = a[j + delta];
        __syncthreads();
        if (j < n) a[j] = v;
    }
}

__global__ __launch_bounds__(256) void k_rt_varresample(RtVarParams p) {
    __shared__ float2 wt[kVarWinLen];
    const int tid = threadIdx.x;
    float* row = p.row + (long long)blockIdx.x * p.ld_row;
    float* outc = p.out + (long long)blockIdx.x * p.ldo;
    long long* ring = p.ring + (long long)blockIdx.x * p.ring_cap;
    const RtMapState st = p.st[blockIdx.x];  // (one address: uniform over the workgroup)
    for (int v = tid; v < kVarWinLen; v += 256) wt[v] = p.win[v];
    __syncthreads();

    const float* x0 = row + p.K;
    long long T = st.rpos;
    int emitted = st.emitted, used = 0;
    for (int k = 0; k < p.nframes; ++k) {
        float* ob = outc + (long long)k * p.hop;
        if (emitted <= p.G) {  // a block below 0
            for (int j = tid; j < p.hop; j += 256) ob[j] = 0.0f;
            ++emitted;
            continue;
        }
        // the block's record {T, d, Sq, W}: pvtab::var_block_filter's operations, IEEE fp64
        const long long d = ring[used++];
        const double v = p.rolloff * fmin(1.0, 4294967296.0 / (double)d) * 4294967296.0;
        const unsigned Sq = (unsigned)floor(v) & ~1u;
        const int W = (int)ceil(p.Z / ((double)Sq / 4294967296.0));
        for (int j = tid; j < p.hop; j += 256) {
            const long long t = T + (long long)j * d;
            ob[j] = vartap::output(x0 + (int)(t >> 32), wt, (unsigned)t, Sq, W, p.win_scale);
        }
        T += (long long)p.hop * d;
    }
    __syncthreads();  // every read of the row and of the ring is done
    // the next block starts inside [row[K], row[K + 1]): what lies more than K below it leaves
    const int delta = (int)(T >> 32);
    const int left = st.fill - delta;  // (>= 0: the next block starts below what is final)
    if (delta > 0) move_down(row, p.K + left, delta, tid);
    const int rest = st.nsteps - used;
    if (used > 0) move_down(ring, rest, used, tid);
    if (tid == 0) {
        RtMapState* sg = p.st + blockIdx.x;
        sg->rpos = T & 0xffffffffLL;
        sg->fill = left;
        sg->nsteps = rest;
        sg->emitted = emitted;
    }
}

bool rt_map_kernel(int L) { return L == 128 || L == 256 || L == 512 || L == 1024; }

hipError_t launch_rt_map(int L, int lock, const RtMapParams& p, hipStream_t s) {
    const int W = L <= 512 ? 4 : 2;
    dim3 grid((p.rt.channels + W - 1) / W), block(64 * W);
#define PV_RT_MAP_L(LL_)                                                                                    \
    if (lock) hipLaunchKernelGGL((k_rt_map<LL_, true>), grid, block, RtMapGeo<LL_>::BYTES, s, p);           \
    else hipLaunchKernelGGL((k_rt_map<LL_, false>), grid, block, RtMapGeo<LL_>::BYTES, s, p);
    switch (L) {
        case 128: PV_RT_MAP_L(128); break;
        case 256: PV_RT_MAP_L(256); break;
        case 512: PV_RT_MAP_L(512); break;
        case 1024: PV_RT_MAP_L(1024); break;
        default: return hipErrorInvalidValue;
    }
#undef PV_RT_MAP_L
    return hipGetLastError();
}

hipError_t launch_rt_varresample(const RtVarParams& p, hipStream_t s) {
    if (p.channels <= 0 || p.nframes <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rt_varresample, dim3((unsigned)p.channels), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace pv
