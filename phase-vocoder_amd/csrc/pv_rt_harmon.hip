// pv_rt_harmon.hip — the real-time harmoniser (pv_rt_harmonizer_push): V voices
// of the real-time pitch map (pv_rt_pitchmap.hip, §3.16) per channel from one analysis, each with
// its own fp32 pitch ratio and gain per pushed frame, mixed on the way out.  Two launches per
// callback, whatever V is:
//
//   k_rt_hmap       a workgroup per channel, a wave per voice (64 V threads).  Per pushed frame
//                   wave 0 analyses the frame — k_rt_map's analysis, operation for operation, so the
//                   row's phases are the oracle's bit for bit — into the channel's LDS row; after a
//                   barrier every wave runs k_rt_map's span loop for its own voice (its own step d,
//                   offset, Phi, FFT tile and overlap accumulator; 0 to 4 stretched frames, no
//                   barrier inside), appends the completed hops to its own scratch row and pushes
//                   {d, gain} into its own ring; a second barrier keeps the next frame's analysis
//                   from overwriting the older row while a voice still reads it.  Every wave
//                   executes the same barriers — one after the tables are loaded, two per pushed
//                   frame — and none leaves early.  A NaN gain is stored as 0.
//   k_rt_hresample  a workgroup per channel, as k_rt_varresample.  Per output block and sample, the
//                   voices in rising order: voice v's sample by vartap::output from its own row with
//                   its own step (Sq, W in fp64 as there), g_v(j) the linear ramp from the previous
//                   block's gain, mix = fmaf(g_v(j), y_v, mix) in a register from +0; the voice's
//                   own sample is stored too when asked for.  Then every voice's row and ring are
//                   compacted as k_rt_varresample compacts them.
//
// There is no dry path: a voice at ratio 1 is the input behind the common latency (G + 1) hop
// (§3.12: the identity map), which is how a caller adds the dry signal aligned with the wet one.
//
// Between launches: per channel the input history and the previous row; per (channel, voice) Phi,
// the overlap accumulator, RtMapState, the ring, the scratch row and the last emitted gain.
//
// A kernel file of its own, so every other kernel keeps its code.
#include "pv_frame.hpp"
#include "pv_kernels.h"
#include "pv_varresample.hpp"

namespace pv {

// LDS of k_rt_hmap, floats: the channel's tables, input window and two rows, then per voice wave an
// FFT tile and an overlap accumulator
template <int L>
struct RtHGeo {
    static constexpr int N = 2 * L;
    static constexpr int B = L + 1;
    static constexpr int VMAX = (L <= 512) ? 8 : 4;
    static constexpr int TILE = Geo<L>::TILE;
    static constexpr int RB = B + 1;                        // float2 slots of a row (even)
    static constexpr int O_TW = 0;                          // L float2
    static constexpr int O_TWS = O_TW + 2 * L;              // L+1 float2 (+1 pad)
    static constexpr int O_WIN = O_TWS + 2 * (L + 2);       // N
    static constexpr int O_GAIN = O_WIN + N;                // N
    static constexpr int O_BUF = O_GAIN + N;                // N input window
    static constexpr int O_ROWS = O_BUF + N;                // 2 x RB float2 {mag, bits of P}
    static constexpr int O_VOICE = O_ROWS + 2 * 2 * RB;     // V x {TILE float2, N overlap accumulator}
    static constexpr int PER = 2 * TILE + N;
    static_assert(O_ROWS % 2 == 0 && O_VOICE % 2 == 0 && PER % 2 == 0, "float2 regions are 8-byte aligned");
    static constexpr size_t bytes(int voices) { return sizeof(float) * (size_t)(O_VOICE + voices * PER); }
    static_assert(bytes(VMAX) <= 160 * 1024, "one workgroup's LDS");
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
__global__ __launch_bounds__(64 * RtHGeo<L>::VMAX) void k_rt_hmap(RtHMapParams pp) {
    using G_ = Geo<L>;
    using R_ = RtHGeo<L>;
    constexpr int MODE = LOCKED ? kModeLockedMap : kModeMap;
    constexpr int E = G_::E;
    constexpr int N = R_::N;
    constexpr int B = R_::B;
    constexpr int SPW = N / 64;
    static_assert(!LOCKED || 2 * R_::TILE >= L + 2, "theta scratch of the locked step: L + 2 floats");
    const RtParams& p = pp.rt;
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float2* twl = reinterpret_cast<float2*>(hsm + R_::O_TW);
    float2* twsl = reinterpret_cast<float2*>(hsm + R_::O_TWS);
    float* winl = hsm + R_::O_WIN;
    float* gainl = hsm + R_::O_GAIN;
    float* buf = hsm + R_::O_BUF;
    float2* rows = reinterpret_cast<float2*>(hsm + R_::O_ROWS);

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's voice (wave-uniform)
    const int V = pp.voices;                                 // (= blockDim.x / 64)
    const int nt = 64 * V;
    const int c = blockIdx.x;                                // (the grid is the channels: no wave leaves early)
    const int hop = p.hop;
    const int keep = N - hop;  // history samples carried to the next frame, and overlap samples
    float2 tw0[E];
    load_tw0<L>(tw0, p.tw);
    float* hist = p.hist + (long long)c * N;
    float2* prevg = pp.prev + (long long)c * p.bins_pad;
    for (int i = tid; i < L; i += nt) twl[i] = p.tw[i];
    for (int i = tid; i < B; i += nt) { twsl[i] = p.tws[i]; rows[i] = prevg[i]; }
    for (int i = tid; i < N; i += nt) { winl[i] = p.win[i]; gainl[i] = p.gain[i]; }
    for (int j = tid; j < keep; j += nt) buf[j] = hist[j];

    // ---- the voice's own state
    const long long cv = (long long)c * V + w;
    float2* tile = reinterpret_cast<float2*>(hsm + R_::O_VOICE + w * R_::PER);
    float* olab = hsm + R_::O_VOICE + w * R_::PER + 2 * R_::TILE;
    float* olag = pp.ola + cv * N;
    for (int j = lane; j < N; j += 64) olab[j] = (j < keep) ? olag[j] : 0.0f;
    int M[E + 1];          // Phi, a 32-bit fraction of a turn per bin (synth_frame's map modes)
    float unused[E + 1];   // (the map modes keep no unwrap state)
    {
        const unsigned* Fg = pp.phi + cv * p.bins_pad;
        PV_FOR_BINS(E, lane, { M[i] = (int)Fg[k]; unused[i] = 0.0f; })
    }
    int cur = 0;  // the half of `rows` that holds the previous row (uniform over the workgroup)
    const RtMapState st = pp.st[cv];
    long long off = uniform64(st.off);
    int fill = __builtin_amdgcn_readfirstlane(st.fill);
    int nsteps = __builtin_amdgcn_readfirstlane(st.nsteps);
    int have = __builtin_amdgcn_readfirstlane(st.rows);
    RtHStep* ringc = pp.ring + cv * pp.ring_cap;
    float* rowg = pp.row + cv * pp.ld_row + pp.K;
    const long long unit = (long long)hop << 32;  // a stretched frame's hop, 2^-32 samples
    const PhaseMap pmap{};
    const SynLds stb{twl, twsl, nullptr, nullptr, nullptr};
    const float* inc = p.in + (long long)c * p.ldi;
    const long long ctl = cv * pp.ld_ctl;
    __syncthreads();  // the tables, the history and the previous row are in LDS

    for (int f = 0; f < p.nframes; ++f) {
        float2 z[E];
        float2* rp = rows + cur * R_::RB;        // row b
        float2* rn = rows + (cur ^ 1) * R_::RB;  // row b + 1, analysed now
        if (w == 0) {
            for (int j = lane; j < hop; j += 64) buf[keep + j] = inc[(long long)f * hop + j];
            wave_lds_sync();
            // ---- analysis (k_rt_map's: the same operations as k_std_analysis)
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
        __syncthreads();  // row b + 1 is written: every voice reads it
        // ---- the voice's step and gain: the ratio clamped with minNum / maxNum (a NaN reads as
        // ratio_min), a NaN gain reads as 0
        const float rq = pp.ratio ? pp.ratio[ctl + f] : 1.0f;
        const float rv = (rq == rq) ? rq : pp.ratio_min;  // (a signalling NaN too)
        const float rc = __builtin_fminf(__builtin_fmaxf(rv, pp.ratio_min), pp.ratio_max);
        const long long d = uniform64((long long)(rc * 0x1p32f));
        const float gq = pp.gain ? pp.gain[ctl + f] : 1.0f / (float)V;
        const float gv = (gq == gq) ? gq : 0.0f;
        if (have == 0) {
            // the stream's first row: Phi(0) = P(0); its ratio and gain are read and ignored
            PV_FOR_BINS(E, lane, { M[i] = (int)__float_as_uint(lds_ld(&rn[k]).y); })
            have = 1;
            off = 0;
        } else {
            const long long span = (long long)hop * d;  // Sigma_{b+1} - Sigma_b
            while (off < span) {  // (0 to 4 rounds, differing between the waves: no barrier inside)
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
            if (lane == 0) { ringc[nsteps].d = d; ringc[nsteps].gain = gv; }  // (nsteps < ring_cap: at most G wait between callbacks)
            ++nsteps;
        }
        cur ^= 1;
        __syncthreads();  // every voice is done with row b: the next analysis overwrites it
    }
    // ---- state back to HBM
    if (w == 0) {  // (the rows and the window are wave 0's own writes)
        for (int j = lane; j < keep; j += 64) hist[j] = buf[j];
        const float2* rl = rows + cur * R_::RB;
        PV_FOR_BINS(E, lane, { prevg[k] = lds_ld(&rl[k]); })
    }
    for (int j = lane; j < keep; j += 64) olag[j] = olab[j];
    {
        unsigned* Fg = pp.phi + cv * p.bins_pad;
        PV_FOR_BINS(E, lane, { Fg[k] = (unsigned)M[i]; })
    }
    if (lane == 0) {  // (rpos and emitted are k_rt_hresample's)
        RtMapState* sg = pp.st + cv;
        sg->off = off;
        sg->rows = have;
        sg->fill = fill;
        sg->nsteps = nsteps;
    }
}

namespace {
// a[j] = a[j + delta], j < n, delta > 0: by the whole workgroup, 256 elements at a time through
// registers (k_rt_varresample's move).  A chunk's writes [j0, j0 + 256) lie below the reads of
// every later chunk (>= j0 + 256 + delta), so one barrier per chunk, between its reads and its
// writes, orders all.
static_assert(sizeof(RtHStep) == sizeof(int4), "the ring moves as 16-byte records");
template <typename T>
__device__ __forceinline__ void hmove_down(T* a, int n, int delta, int tid) {
    for (int j0 = 0; j0 < n; j0 += 256) {  // (uniform bound: every thread reaches the barrier)
        const int j = j0 + tid;
        T v{};
        if (j < n) v = a[j + delta];
        __syncthreads();
        if (j < n) a[j] = v;
    }
}
}  // namespace

__global__ __launch_bounds__(256) void k_rt_hresample(RtHVarParams p) {
    __shared__ float2 wt[kVarWinLen];
    __shared__ long long Tl[kRtHarmonMaxVoices];   // start of the voice's next block
    __shared__ float gpl[kRtHarmonMaxVoices];      // the voice's last emitted gain ...
    __shared__ int gpl_have[kRtHarmonMaxVoices];   // ... if a block has been emitted
    __shared__ int filll[kRtHarmonMaxVoices], nstepsl[kRtHarmonMaxVoices];
    __shared__ int emittedl;
    const int tid = threadIdx.x;
    const int V = p.voices;
    const long long c = blockIdx.x;
    float* mixc = p.mix + c * p.ldo;
    for (int v = tid; v < kVarWinLen; v += 256) wt[v] = p.win[v];
    if (tid < V) {
        const RtMapState* sg = p.st + c * V + tid;
        Tl[tid] = sg->rpos;
        filll[tid] = sg->fill;
        nstepsl[tid] = sg->nsteps;
        if (tid == 0) emittedl = sg->emitted;
        gpl[tid] = p.gprev[c * V + tid].g;
        gpl_have[tid] = p.gprev[c * V + tid].have;
    }
    __syncthreads();

    const float inv_hop = 1.0f / (float)p.hop;
    // (every voice has been pushed the same frames: one count of emitted blocks and of used steps)
    int emitted = emittedl, used = 0;
    for (int k = 0; k < p.nframes; ++k) {
        float* ob = mixc + (long long)k * p.hop;
        if (emitted <= p.G) {  // a block below 0 (uniform over the workgroup)
            for (int j = tid; j < p.hop; j += 256) {
                ob[j] = 0.0f;
                if (p.voices_out != nullptr)
                    for (int v = 0; v < V; ++v) p.voices_out[(v * (long long)p.channels + c) * p.ld_voice + (long long)k * p.hop + j] = 0.0f;
            }
            ++emitted;
        } else {
            for (int j = tid; j < p.hop; j += 256) {
                float acc = 0.0f;
                const float fr = (float)(j + 1) * inv_hop;
                for (int v = 0; v < V; ++v) {
                    const long long cv = c * V + v;
                    // the block's record {T, d, Sq, W}: pvtab::var_block_filter's operations, IEEE fp64
                    const RtHStep* sr = p.ring + cv * p.ring_cap + used;
                    const long long d = sr->d;
                    const float gb = sr->gain;
                    const double q = p.rolloff * fmin(1.0, 4294967296.0 / (double)d) * 4294967296.0;
                    const unsigned Sq = (unsigned)floor(q) & ~1u;
                    const int W = (int)ceil(p.Z / ((double)Sq / 4294967296.0));
                    const float* x0 = p.row + cv * p.ld_row + p.K;
                    const long long t = Tl[v] + (long long)j * d;
                    const float y = vartap::output(x0 + (int)(t >> 32), wt, (unsigned)t, Sq, W, p.win_scale);
                    // the gain's ramp from the previous block's (block 0: from its own)
                    const float g0 = gpl_have[v] ? gpl[v] : gb;
                    const float g = __builtin_fmaf(fr, gb - g0, g0);
                    acc = __builtin_fmaf(g, y, acc);
                    if (p.voices_out != nullptr)
                        p.voices_out[(v * (long long)p.channels + c) * p.ld_voice + (long long)k * p.hop + j] = y;
                }
                ob[j] = acc;
            }
            __syncthreads();  // the block's reads of Tl and the gains are done
            if (tid < V) {
                const RtHStep* sr = p.ring + (c * V + tid) * p.ring_cap + used;
                Tl[tid] += (long long)p.hop * sr->d;
                gpl[tid] = sr->gain;
                gpl_have[tid] = 1;
            }
            ++used;
            __syncthreads();
        }
    }
    __syncthreads();  // every read of the rows and of the rings is done
    for (int v = 0; v < V; ++v) {
        const long long cv = c * V + v;
        // the next block starts inside [row[K], row[K + 1]): what lies more than K below it leaves
        const long long T = Tl[v];
        const int delta = (int)(T >> 32);
        const int left = filll[v] - delta;  // (>= 0: the next block starts below what is final)
        if (delta > 0) hmove_down(p.row + cv * p.ld_row, p.K + left, delta, tid);
        const int rest = nstepsl[v] - used;
        if (used > 0) hmove_down(reinterpret_cast<int4*>(p.ring + cv * p.ring_cap), rest, used, tid);  // (16-byte records)
        if (tid == 0) {
            RtMapState* sg = p.st + cv;
            sg->rpos = T & 0xffffffffLL;
            sg->fill = left;
            sg->nsteps = rest;
            sg->emitted = emitted;
            p.gprev[cv].g = gpl[v];
            p.gprev[cv].have = gpl_have[v];
        }
    }
}

int rt_hmap_max_voices(int L) { return (L == 128 || L == 256 || L == 512) ? 8 : (L == 1024) ? 4 : 0; }

hipError_t launch_rt_hmap(int L, int lock, const RtHMapParams& p, hipStream_t s) {
    if (p.rt.channels <= 0 || p.voices < 1 || p.voices > rt_hmap_max_voices(L)) return hipErrorInvalidValue;
    dim3 grid((unsigned)p.rt.channels), block(64 * p.voices);
#define PV_RT_HMAP_L(LL_)                                                                                         \
    if (lock) hipLaunchKernelGGL((k_rt_hmap<LL_, true>), grid, block, RtHGeo<LL_>::bytes(p.voices), s, p);        \
    else hipLaunchKernelGGL((k_rt_hmap<LL_, false>), grid, block, RtHGeo<LL_>::bytes(p.voices), s, p);
    switch (L) {
        case 128: PV_RT_HMAP_L(128); break;
        case 256: PV_RT_HMAP_L(256); break;
        case 512: PV_RT_HMAP_L(512); break;
        case 1024: PV_RT_HMAP_L(1024); break;
        default: return hipErrorInvalidValue;
    }
#undef PV_RT_HMAP_L
    return hipGetLastError();
}

hipError_t launch_rt_hresample(const RtHVarParams& p, hipStream_t s) {
    if (p.channels <= 0 || p.nframes <= 0 || p.voices < 1 || p.voices > kRtHarmonMaxVoices) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rt_hresample, dim3((unsigned)p.channels), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace pv
