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

// ---- one output's taps (device code).  No coefficient table can exist (the phase is arbitrary), so
// every tap's h = sin(pi s tau) / (pi tau) * win(s tau / Z) is computed; pv_varresample.hip's header
// has the derivation.  k_var_resample and the real-time k_rt_varresample (pv_rt_pitchmap.hip) share
// the sines; `output` is the streaming kernel's form of k_var_resample's tap loop, the same
// operations in the same order (the batched kernel keeps the loop in its own body: called from
// here the compiler swaps the operands of some of its multiplies, scripts/asm_diff.py).
namespace vartap {

constexpr float kPiF = 0x1.921fb6p+1f;
constexpr float kTwoPiF = 0x1.921fb6p+2f;

// sin(a), |a| <= pi/2: the odd Taylor polynomial of degree 11 (its next term is 5.7e-8 at pi/2)
__device__ __forceinline__ float sin_folded(float a) {
    const float a2 = a * a;
    float c = -0x1.ae6456p-26f;         // -1 / 11!
    c = fmaf(c, a2, 0x1.71de3ap-19f);   //  1 / 9!
    c = fmaf(c, a2, -0x1.a01a02p-13f);  // -1 / 7!
    c = fmaf(c, a2, 0x1.111112p-7f);    //  1 / 5!
    c = fmaf(c, a2, -0x1.555556p-3f);   // -1 / 3!
    return fmaf(a2 * a, c, a);
}
// sin(2 pi p / 2^32).  sin(pi - a) = sin(a): a phase in the second or third quarter turn is
// folded about the quarter turn in integers; the angle then lies in [-pi/2, pi/2].
__device__ __forceinline__ float sin_turn(unsigned p) {
    const unsigned q = (p + 0x40000000u) >= 0x80000000u ? 0x80000000u - p : p;
    return sin_folded((float)(int)q * (kTwoPiF * 0x1p-32f));
}
// the same of p / 2^64, for the two taps next to the centre: |tau| may be tiny there, and the
// angle keeps its relative precision only if the conversion to fp32 sees all 64 bits
__device__ __forceinline__ float sin_turn64(unsigned long long p) {
    const unsigned long long q = (p + (1ull << 62)) >= (1ull << 63) ? (1ull << 63) - p : p;
    return sin_folded((float)(long long)q * (kTwoPiF * 0x1p-64f));
}

// The output at the fraction fq / 2^32 past x[i], xc = &x[i]: the taps reach xc[-W + 1 .. W], in
// rising order into one fp32 sum.  wt: the window table (kVarWinLen entries), win_scale as in
// VarResampleParams.
__device__ __forceinline__ float output(const float* xc, const float2* wt, unsigned fq, unsigned Sq, int W,
                                        float win_scale) {
    const unsigned hS = Sq >> 1;
    // top 32 bits of -(hS fq) modulo 2^64, rounded down
    const unsigned long long prod = (unsigned long long)hS * fq;
    const unsigned a0 = 0u - (unsigned)(prod >> 32) - ((unsigned)prod != 0u ? 1u : 0u);
    const float f = (float)fq * 0x1p-32f;                           // the fraction
    const float g = fq ? (float)(0u - fq) * 0x1p-32f : 1.0f;        // 1 - fraction
    const float sq = (float)Sq;
    const float s = sq * 0x1p-32f;
    const float ws = sq * win_scale;
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
    return acc;
}

}  // namespace vartap

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
