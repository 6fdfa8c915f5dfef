// pv_resample.hpp — band-limited polyphase resampler (pv_resample, pv_pitch_process; DESIGN.md
// §3.8): the kernel's parameter block, its tile plan and its launcher.
//
// Output m of a P:Q resampler (reduced) reads the input at m P / Q: integer part i_m, phase
// r_m = (m P) mod Q, y[m] = sum_{t < 2W} x[i_m - W + 1 + t] c[r_m][t], where c[r][t] =
// h(t - W + 1 - r / Q) is the Kaiser-windowed sinc of include/pv.h.  Outputs m and m + D share
// their coefficients when Q divides D, and their input windows are D P / Q samples apart.
#pragma once
#include <hip/hip_runtime.h>

namespace pv {

// How a workgroup's tile is cut (made once per resampler by resample_plan).  A tile is R * D
// consecutive outputs of one channel; a thread takes the outputs u, u + 1 and their R - 1
// repeats D, 2 D, .. further on (u even, u < D, in steps of 512).  The repeats of an output share
// its coefficient row, and the neighbours u, u + 1 share their input slots.  For R > 1, D is a
// multiple of 4 Q: the R input windows then start a multiple of 4 samples apart, so that every
// one of them has the same offset in its aligned 16-byte LDS slot.
struct ResamplePlan {
    int R;      // outputs per coefficient read: 8, 4, 2 or 1
    int D;      // outputs between two outputs of one phase of a thread (even)
    int W;      // half width of the filter: taps t = 0 .. 2W - 1
    int NC;     // 16-byte slots a thread's two windows can touch: ceil((2W + 7) / 4)
    int span4;  // 16-byte slots of input a tile stages in LDS
};

// The coefficient table in its eight alignments, float4 tab[(off * Q + r) * NC + c], off < 8:
// element e = 4 c + lane-of-float4 holds c[r][e - off], or 0 outside [0, 2W): a window that starts
// `off` floats after an aligned slot multiplies whole slots (off < 4: its own first slot; up to
// 7: the slot of its lower neighbour, at most ceil(P / Q) <= 4 samples before).
struct ResampleParams {
    const float* x;
    long long ldx, n_in;
    float* y;
    long long ldy, n_out;
    const float4* tab;
    int P, Q;
    ResamplePlan plan;
    int ntiles;  // tiles per channel: grid.x = ntiles * channels
};

// LDS bytes a plan may ask for (three workgroups per CU)
constexpr int kResampleLdsBytes = 48 * 1024;

bool resample_plan(int P, int Q, int W, ResamplePlan* plan);
hipError_t launch_resample(int channels, const ResampleParams& p, hipStream_t s);
// rows copied as they are (ratio 1)
hipError_t launch_copy_rows(const float* x, long long ldx, float* y, long long ldy, long long n, int channels,
                            hipStream_t s);

}  // namespace pv
