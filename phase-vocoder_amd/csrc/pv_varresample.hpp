// pv_varresample.hpp — band-limited resampler whose ratio changes along the signal
// (pv_varresample, pv_pitchmap_process): the per-block and per-tile records the
// host builds, the kernel's parameter block and its launchers.
//
// The output is cut into blocks of B samples.  Block b starts at the input position T_b (64-bit,
// units of 2^-32 samples) and steps by d_b per output: output m = b B + j reads at
// t = T_b + j d_b, i = t >> 32, fq = (unsigned)t, through the Kaiser-windowed sinc of include/pv.h
// whose cutoff s_b = Sq_b / 2^32 and half width W_b are the block's.  The phase is arbitrary, so
// no coefficient table exists: every tap's coefficient is computed (pv_varresample.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pv {

struct VarBlock {
    long long T;  // position of the block's first output
    long long d;  // step per output, 2^30 .. 2^34
    unsigned Sq;  // cutoff s = Sq / 2^32 (even)
    int W;        // half width: taps j = -W + 1 .. W
};

// A tile is kVarTile consecutive outputs of one channel, whatever B.  Its outputs read the input
// samples base .. base + span - 1; the workgroup stages 4 span4 >= span + 3 floats from the
// 16-byte boundary at or below `base`.
struct VarTile {
    long long base;
    int span4;
    int pad_;
};

constexpr int kVarTile = 1024;
// The window table, with the 1 / pi of the sinc folded in: kVarWinN intervals over |u| in [0, 1],
// float2 {w(i / n) / pi, the rise to the next entry} for i < n, then {0, 0} (|u| >= 1) up to
// kVarWinLen entries: a tap's |u| = s |tau| / Z is below W s / Z < 1 + s / Z <= 1 + 1 / 16
// (W = ceil(Z / s), s < 1, Z >= 16), so its index needs no clamp.
constexpr int kVarWinN = 2048;
constexpr int kVarWinLen = kVarWinN + kVarWinN / 16 + 2;

struct VarResampleParams {
    const float* x;
    long long ldx, n_in;
    float* y;
    long long ldy, n_out;
    const VarBlock* blocks;
    const VarTile* tiles;
    // maps per channel (pv_varresampler_set_maps): channel c reads blocks +
    // c * ld_blocks and tiles + c * ld_tiles (0: one map for all channels).  copy_shift (nullptr
    // for the shared map): per channel the shift of a channel that is a copy, y[m] = x[shift + m],
    // or -1 for a filtered one
    long long ld_blocks, ld_tiles;
    const long long* copy_shift;
    const float2* win;
    int B;
    int ntiles;       // tiles per channel: grid.x = ntiles * channels
    float win_scale;  // kVarWinN / Z * 2^-32: (float)Sq * win_scale * |tau| indexes the window table
};

// span4_max: the largest span4 of the map's tiles, over the channels (the launch's dynamic LDS)
hipError_t launch_var_resample(int channels, const VarResampleParams& p, int span4_max, hipStream_t s);
// every step 2^32 and no fraction: y[m] = x[shift + m], 0 past n_in; shifts: one per channel
// (nullptr: `shift` for all)
hipError_t launch_var_copy(const float* x, long long ldx, long long n_in, long long shift, const long long* shifts,
                           float* y, long long ldy, long long n_out, int channels, hipStream_t s);

}  // namespace pv
