// pv_resample.hip — band-limited polyphase resampler (pv_resample, pv_pitch_process; DESIGN.md
// §3.8).
//
//   k_resample<R>   one launch over channels x output tiles.  A workgroup stages its tile's input
//                   span in LDS (16-byte loads and LDS writes, masked at [0, n_in)) and every
//                   thread forms 2 R outputs, R of each of two neighbouring phases: per 16-byte
//                   slot of the filter it reads 4 coefficients of either phase once (two float4
//                   from the cached table) and R aligned float4 of input from LDS, which both
//                   phases use, for 8 R fused multiply-adds.
//   k_copy_rows     ratio 1: the rows as they are.
//
// No state, no allocation, no synchronisation: capturable.  A kernel file of its own, so every
// other kernel keeps its code.
#include <cstdint>

#include "pv_resample.hpp"

namespace pv {

// outputs of neighbouring phases per thread: their windows start within 8 samples of one
// aligned slot (ratios up to 4), so they share the R input slots of every step
constexpr int kA = 2;

// (clang vector types: an element-wise fma of two floats is one v_pk_fma_f32 on operands that
// sit in neighbouring registers as loaded)
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

template <int R>
__global__ __launch_bounds__(256) void k_resample(ResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) f4 xs[];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % p.ntiles, ch = blockIdx.x / p.ntiles;
    const int P = p.P, Q = p.Q, W = p.plan.W, NC = p.plan.NC, D = p.plan.D;
    const long long m0 = (long long)tile * ((long long)R * D);
    const long long pos0 = m0 * P;
    const long long i0 = pos0 / Q;
    const int r0 = (int)(pos0 - i0 * Q);
    const float* row = p.x + (long long)ch * p.ldx;
    // the staged span starts at the first sample of output m0's window, moved down by `mis` < 4
    // samples to a 16-byte boundary of global memory (whatever the row's own alignment)
    const long long base0 = i0 - W + 1;
    const int mis = (int)(((long long)(reinterpret_cast<uintptr_t>(row) >> 2) + base0) & 3);
    const long long abase = base0 - mis;
    for (int v = tid; v < p.plan.span4; v += 256) {
        const long long g = abase + 4LL * v;
        f4 q;
        if (g >= 0 && g + 3 < p.n_in) {
            q = *reinterpret_cast<const f4*>(row + g);
        } else {  // x reads as 0 outside [0, n_in)
            q.x = (g >= 0 && g < p.n_in) ? row[g] : 0.0f;
            q.y = (g + 1 >= 0 && g + 1 < p.n_in) ? row[g + 1] : 0.0f;
            q.z = (g + 2 >= 0 && g + 2 < p.n_in) ? row[g + 2] : 0.0f;
            q.w = (g + 3 >= 0 && g + 3 < p.n_in) ? row[g + 3] : 0.0f;
        }
        xs[v] = q;
    }
    __syncthreads();

    // 16-byte slots between the windows of two outputs of one phase (R > 1: D P / Q is a
    // multiple of 4, resample_plan)
    const int stepk = (R > 1) ? (int)(((long long)D * P / Q) >> 2) : 0;
    float* yrow = p.y + (long long)ch * p.ldy;
    for (int u = kA * tid; u < D; u += kA * 256) {
        const long long m = m0 + u;
        if (m >= p.n_out) break;
        // output m0 + u + a sits (r0 + (u + a) P) / Q samples after i0; the remainder is its phase
        int c0 = 0;
        const f4* trow[kA];
#pragma unroll
        for (int a = 0; a < kA; ++a) {
            const unsigned n = (unsigned)r0 + (unsigned)(u + a) * (unsigned)P;
            const unsigned di = n / (unsigned)Q;
            const int r = (int)(n - di * (unsigned)Q);
            const int rel = (int)di + mis;  // first sample of the window, in staged samples
            if (a == 0) c0 = rel >> 2;
            const int off = rel - 4 * c0;   // 0 .. 7
            trow[a] = reinterpret_cast<const f4*>(p.tab) + ((size_t)off * Q + r) * NC;
        }
        // two partial sums per output: the even and the odd taps
        f2 acc[kA][R];
#pragma unroll
        for (int a = 0; a < kA; ++a)
#pragma unroll
            for (int k = 0; k < R; ++k) acc[a][k] = f2{0.0f, 0.0f};
#pragma unroll 2
        for (int c = 0; c < NC; ++c) {
            f4 h[kA];
#pragma unroll
            for (int a = 0; a < kA; ++a) h[a] = trow[a][c];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const f4 xv = xs[c0 + k * stepk + c];
#pragma unroll
                for (int a = 0; a < kA; ++a) {
                    acc[a][k] = __builtin_elementwise_fma(h[a].xy, xv.xy, acc[a][k]);
                    acc[a][k] = __builtin_elementwise_fma(h[a].zw, xv.zw, acc[a][k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int a = 0; a < kA; ++a) {
                const long long mk = m + a + (long long)k * D;
                if (mk < p.n_out) yrow[mk] = acc[a][k].x + acc[a][k].y;
            }
    }
}

// The tile plan.  R = 8, 4, else 2: D = 4 Q c, the c whose D / 2 fills whole 256-thread passes
// best among those whose tile fits the LDS budget (D >= 512 preferred: a longer tile carries
// less halo); R = 1 (any P, Q in the accepted range): tiles of 1024 outputs.
bool resample_plan(int P, int Q, int W, ResamplePlan* plan) {
    const int cap4 = kResampleLdsBytes / 16;
    // a window starts at most ceil(T P / Q) + 3 samples into the span; the thread's first
    // window's slot and the NC - 1 after it end at most 4 NC - 1 <= 2W + 9 samples later
    auto span4_of = [&](long long T) { return (int)((((T * P + Q - 1) / Q) + 2 * W + 16 + 3) / 4); };
    plan->W = W;
    plan->NC = (2 * W + 7 + 3) / 4;
    for (int R = 8; R >= 2; R /= 2) {
        double best = -1.0;
        long long bestD = 0;
        for (long long c = 1;; ++c) {
            const long long D = 4LL * Q * c;
            if (D > 65536 || span4_of(R * D) > cap4) break;
            const long long passes = (D / kA + 255) / 256;
            const double eff = (double)(D / kA) / (256.0 * (double)passes);
            const double score = eff - (D < 512 ? 0.02 : 0.0);
            if (score > best + 1e-9) {
                best = score;
                bestD = D;
            }
            if (D >= 512 && eff >= 0.995) break;
        }
        if (best >= 0.6) {
            plan->R = R;
            plan->D = (int)bestD;
            plan->span4 = span4_of(R * bestD);
            return true;
        }
    }
    plan->R = 1;
    plan->D = 1024;
    plan->span4 = span4_of(1024);
    return plan->span4 <= cap4;
}

hipError_t launch_resample(int channels, const ResampleParams& p, hipStream_t s) {
    if ((long long)p.ntiles * channels > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(p.ntiles * channels));
    const size_t lds = sizeof(float4) * (size_t)p.plan.span4;
    switch (p.plan.R) {
        case 8: hipLaunchKernelGGL(k_resample<8>, grid, dim3(256), lds, s, p); break;
        case 4: hipLaunchKernelGGL(k_resample<4>, grid, dim3(256), lds, s, p); break;
        case 2: hipLaunchKernelGGL(k_resample<2>, grid, dim3(256), lds, s, p); break;
        case 1: hipLaunchKernelGGL(k_resample<1>, grid, dim3(256), lds, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_copy_rows(const float* x, long long ldx, float* y, long long ldy,
                                                   long long n, int ntiles) {
    const int tile = blockIdx.x % ntiles, ch = blockIdx.x / ntiles;
    const float* src = x + (long long)ch * ldx;
    float* dst = y + (long long)ch * ldy;
    const long long i0 = (long long)tile * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = i0 + 256 * k;
        if (i < n) dst[i] = src[i];
    }
}

hipError_t launch_copy_rows(const float* x, long long ldx, float* y, long long ldy, long long n, int channels,
                            hipStream_t s) {
    const long long ntiles = (n + 1023) / 1024;
    if (ntiles * channels > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)(ntiles * channels)), dim3(256), 0, s, x, ldx, y, ldy, n,
                       (int)ntiles);
    return hipGetLastError();
}

}  // namespace pv
