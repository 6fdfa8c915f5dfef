// pv_varresample.hip — band-limited resampler with a ratio that changes along the signal
// (pv_varresample, pv_pitchmap_process).
//
//   k_var_resample  one launch over channels x tiles of kVarTile consecutive outputs.  A workgroup
//                   stages its tile's input span (the host's VarTile record) in LDS with 16-byte
//                   loads masked at [0, n_in), and the window table beside it; a thread forms the
//                   outputs tid, tid + 256, .. of the tile, each from its own block's record.
//                   No coefficient table can exist (the phase is arbitrary), so every tap's
//                   h = sin(pi s tau) / (pi tau) * win(s tau / Z) is computed:
//                     - the sine's argument as an exact fraction of a turn: with hS = Sq / 2 the
//                       turn count s tau / 2 of tap j is (hS j 2^32 - hS fq) / 2^64 modulo 1; its
//                       top 32 bits are a 32-bit sum that steps by hS per tap, whatever |tau|
//                       (the two taps next to the centre keep all 64 bits: 2^-32 turn over a
//                       tiny tau would be a large relative error);
//                     - the sine from that integer: folded to [-1/4, 1/4] turn exactly, then the
//                       odd polynomial of degree 11 (relative accuracy at small angles, which the
//                       taps next to the centre need: there sin / (pi tau) is a 0/0 form);
//                     - tau from the integers too: j - f for j <= 0 and (j - 1) + (1 - f) for
//                       j >= 1, f and 1 - f each rounded once from fq (no cancellation);
//                     - the Kaiser window by linear interpolation in a table over |u| in [0, 1].
//   k_var_copy      every step 2^32, no fraction: the shifted rows as they are.
// With maps per channel (pv_varresampler_set_maps) a workgroup reads its channel's
// records, and a channel that is a copy beside filtered ones copies its tiles in k_var_resample
// (a test that is uniform over the workgroup): k_var_copy's values, bit for bit.
//
// No state, no allocation, no synchronisation: capturable.  A kernel file of its own, so every
// other kernel keeps its code.
#include <cstdint>

#include "pv_varresample.hpp"

namespace pv {

typedef float f4 __attribute__((ext_vector_type(4)));

using namespace vartap;  // sin_turn, sin_turn64, kPiF (pv_varresample.hpp)

__global__ __launch_bounds__(256) void k_var_resample(VarResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) f4 xs4[];
    __shared__ float2 wt[kVarWinLen];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % p.ntiles, ch = blockIdx.x / p.ntiles;
    const float* row = p.x + (long long)ch * p.ldx;
    if (p.copy_shift) {
        const long long shift = p.copy_shift[ch];  // (uniform over the workgroup, before any barrier)
        if (shift >= 0) {
            float* dst = p.y + (long long)ch * p.ldy;
            for (int k = 0; k < kVarTile / 256; ++k) {
                const long long m = (long long)tile * kVarTile + tid + 256 * k;
                if (m < p.n_out) dst[m] = (shift + m < p.n_in) ? row[shift + m] : 0.0f;
            }
            return;
        }
    }
    const VarTile tr = p.tiles[(long long)ch * p.ld_tiles + tile];
    // the staged span starts at the tile's first input sample, moved down by `mis` < 4 samples to
    // a 16-byte boundary of global memory (whatever the row's own alignment)
    const int mis = (int)(((long long)(reinterpret_cast<uintptr_t>(row) >> 2) + tr.base) & 3);
    const long long abase = tr.base - mis;
    for (int v = tid; v < tr.span4; v += 256) {
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
        xs4[v] = q;
    }
    for (int v = tid; v < kVarWinLen; v += 256) wt[v] = p.win[v];
    __syncthreads();

    const float* xs = reinterpret_cast<const float*>(xs4);
    float* yrow = p.y + (long long)ch * p.ldy;
    const VarBlock* blocks = p.blocks + (long long)ch * p.ld_blocks;
    for (int k = 0; k < kVarTile / 256; ++k) {
        const long long m = (long long)tile * kVarTile + tid + 256 * k;
        if (m >= p.n_out) break;
        const unsigned b = (unsigned)m / (unsigned)p.B;
        const unsigned j = (unsigned)m - b * (unsigned)p.B;
        const VarBlock blk = blocks[b];
        const long long t = blk.T + (long long)j * blk.d;
        const long long i = t >> 32;
        const unsigned fq = (unsigned)t;
        const float* xc = xs + (int)(i - abase);  // x[i]; the taps reach xc[-W + 1 .. W]
        const int W = blk.W;
        const unsigned hS = blk.Sq >> 1;
        // top 32 bits of -(hS fq) modulo 2^64, rounded down
        const unsigned long long prod = (unsigned long long)hS * fq;
        const unsigned a0 = 0u - (unsigned)(prod >> 32) - ((unsigned)prod != 0u ? 1u : 0u);
        const float f = (float)fq * 0x1p-32f;                           // the fraction
        const float g = fq ? (float)(0u - fq) * 0x1p-32f : 1.0f;        // 1 - fraction
        const float sq = (float)blk.Sq;
        const float s = sq * 0x1p-32f;
        const float ws = sq * p.win_scale;
        // win(|u|) / pi: |tau| ws <= kVarWinN (1 + 1 / Z) indexes the table, zeros past |u| = 1
        auto window = [&](float tau) {
            const float tt = __builtin_fabsf(tau) * ws;
            const float2 e = wt[(int)tt];
            return fmaf(__builtin_amdgcn_fractf(tt), e.y, e.x);
        };
        // a tap with |tau| >= 1: x h(tau) + acc, sn = sin(pi s tau)
        auto tap = [&](float tau, float sn, float xv, float acc) {
            return fmaf(xv, (sn * __builtin_amdgcn_rcpf(tau)) * window(tau), acc);
        };
        // taps 0 and 1, |tau| <= 1: tau = 0 (fq = 0 at tap 0) gives h = s
        auto centre = [&](float tau, float sn, float xv, float acc) {
            const float h = tau == 0.0f ? s * kPiF : sn * __builtin_amdgcn_rcpf(tau);
            return fmaf(xv, h * window(tau), acc);
        };
        float acc = 0.0f;
        unsigned ph = a0 + hS * (unsigned)(1 - W);
        for (int jj = 1 - W; jj < 0; ++jj, ph += hS) acc = tap((float)jj - f, sin_turn(ph), xc[jj], acc);
        // the turn count in all its 64 bits (|s tau / 2| < 1/2)
        acc = centre(-f, sin_turn64(0ull - prod), xc[0], acc);
        acc = centre(g, sin_turn64(((unsigned long long)hS << 32) - prod), xc[1], acc);
        ph = a0 + 2u * hS;
        for (int jj = 2; jj <= W; ++jj, ph += hS) acc = tap((float)(jj - 1) + g, sin_turn(ph), xc[jj], acc);
        yrow[m] = acc;
    }
}

hipError_t launch_var_resample(int channels, const VarResampleParams& p, int span4_max, hipStream_t s) {
    if ((long long)p.ntiles * channels > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(p.ntiles * channels));
    hipLaunchKernelGGL(k_var_resample, grid, dim3(256), sizeof(float4) * (size_t)span4_max, s, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_var_copy(const float* x, long long ldx, long long n_in, long long shift,
                                                  const long long* shifts, float* y, long long ldy, long long n_out,
                                                  int ntiles) {
    const int tile = blockIdx.x % ntiles, ch = blockIdx.x / ntiles;
    if (shifts) shift = shifts[ch];
    const float* src = x + (long long)ch * ldx;
    float* dst = y + (long long)ch * ldy;
    const long long m0 = (long long)tile * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long m = m0 + 256 * k;
        if (m < n_out) dst[m] = (shift + m < n_in) ? src[shift + m] : 0.0f;
    }
}

hipError_t launch_var_copy(const float* x, long long ldx, long long n_in, long long shift, const long long* shifts,
                           float* y, long long ldy, long long n_out, int channels, hipStream_t s) {
    const long long ntiles = (n_out + 1023) / 1024;
    if (ntiles * channels > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_var_copy, dim3((unsigned)(ntiles * channels)), dim3(256), 0, s, x, ldx, n_in, shift, shifts, y,
                       ldy, n_out, (int)ntiles);
    return hipGetLastError();
}

}  // namespace pv
