// pv_rt_pitch.hip — streaming band-limited resampler of the real-time pitch shift
// (pv_rt_pitch_push): the second launch of a callback, after k_rt has written
// the callback's nframes * out_hop stretched samples behind the channel's history.
//
//   k_rt_resample   a workgroup per channel.  The channel's scratch row is
//                   [H history | n_new new samples], H >= 2W: output u of the callback reads
//                   2W samples starting H - 2W + 1 + (u P + off) / Q into the row, with the
//                   coefficient row of phase (u P + off) mod Q, off = W Q - D P (pv_kernels.h
//                   RtResampleParams; the bounds are worked out in DESIGN.md §3.9).  The position
//                   is relative to the callback's first stretched sample: no sample counter is
//                   kept, the stream can run for ever.  Then the last H samples of the row move
//                   to its front; the move overlaps its source when n_new < H, and other lanes
//                   read the old history for their outputs, so it is staged in LDS behind a
//                   barrier.
//
// Four neighbouring lanes share an output: lane s takes the taps t = s, s + 4, .. in rising
// order and the partial sums are added as (a0 + a1) + (a2 + a3).  The order depends on nothing
// but the tap index, so a stream gives the same bits however it is cut into callbacks.  A pass
// of the workgroup is 64 outputs — BASELINE config 5's callback (hop 64) exactly.  The samples
// and the coefficients are read from global memory as they are: the row was written by the
// launch before and the table is a few KB per phase set, both sit in L2, and a window's reads
// are consecutive words that neighbouring outputs share.
//
// A kernel file of its own, so every other kernel keeps its code.
#include "pv_kernels.h"

namespace pv {

__global__ __launch_bounds__(256) void k_rt_resample(RtResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) float stage[];  // H floats
    const int tid = threadIdx.x;
    const int sub = tid & 3, slot = tid >> 2;
    float* row = p.row + (long long)blockIdx.x * p.ld_row;
    float* outc = p.out + (long long)blockIdx.x * p.ldo;
    const int taps = 2 * p.W;
    for (int u0 = 0; u0 < p.n_out; u0 += 64) {  // (uniform bound: every lane reaches the exchanges)
        const int u = u0 + slot;
        const bool live = u < p.n_out;
        float acc = 0.0f;
        if (live) {
            const unsigned n = (unsigned)u * (unsigned)p.P + p.off;
            const unsigned di = n / (unsigned)p.Q;
            const unsigned r = n - di * (unsigned)p.Q;
            const float* x = row + (p.H - taps + 1 + (int)di);
            const float* h = p.tab + (size_t)r * (size_t)taps;
#pragma unroll 4
            for (int t = sub; t < taps; t += 4) acc = __builtin_fmaf(x[t], h[t], acc);
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        if (live && sub == 0) outc[u] = acc;
    }
    // the last H samples of [history | new] become the history
    for (int j = tid; j < p.H; j += 256) stage[j] = row[p.n_new + j];
    __syncthreads();  // every lane's window reads and the staging are done
    for (int j = tid; j < p.H; j += 256) row[j] = stage[j];
}

hipError_t launch_rt_resample(const RtResampleParams& p, hipStream_t s) {
    if (p.channels <= 0 || p.n_out <= 0 || p.H < 2 * p.W) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rt_resample, dim3((unsigned)p.channels), dim3(256), sizeof(float) * (size_t)p.H, s, p);
    return hipGetLastError();
}

}  // namespace pv
