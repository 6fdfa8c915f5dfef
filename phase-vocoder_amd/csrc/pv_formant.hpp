// pv_formant.hpp — formant-preserving STANDARD pitch shift (pv_set_formant):
// the pitch gather of one frame in its formant form.  The frame's log envelope le[k] (the
// low-quefrency part of its log magnitude, k_envelope in pv_formant.hip) whitens the source
// bins before the gather and re-colours the gathered sum at the target bin:
//   |Y[k']| = exp(le[k']) * sum over the sources k of k' of mag[k] exp(-le[k]).
// Used by synth_frame's formant mode (pv_frame.hpp) in k_synthesis in the formant mode
// (pv_syn_kernel.hpp, instantiated in pv_formant.hip).
#pragma once
#include "pv_device.hpp"

namespace pv {

// synth_frame / syn_run MODE of the formant-preserving STANDARD pitch shift
constexpr int kModeFormant = 7;

// the frame's envelope row in the caller's registers (v[i]: bin lane + 64 i, v[E]: bin L), or
// none (every other mode)
struct NoEnv {
    static constexpr bool ON = false;
};
template <int E>
struct EnvReg {
    static constexpr bool ON = true;
    float v[E + 1];
};

constexpr float kLog2e = 0x1.715476p+0f;
constexpr float kLn2 = 0x1.62e43p-1f;
// exp by the hardware v_exp_f32 (2^x, 1 ulp): the envelope is tolerance bound
__device__ __forceinline__ float exp_hw(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// A wave holds the frame: bin k = lane + 64 i in register slot i (i < E), bin L in slot E of
// lane 0 (the other lanes' slot E computes bin L too and is ignored).  {mag exp(-le), output
// phase} of every bin goes to the tile (natural order; slot L + 1 takes the other lanes' slot
// E), every bin then reads its {first source, count} from the map, the first source's entry
// in one read (none: zero), further sources (ratios < 1) summed in source order, and scales
// the sum by exp(le) of its own bin.  The LDS reads are issued as batches (all map reads, all
// tile reads, then the arithmetic): the volatile loads keep program order.
template <int L>
__device__ __forceinline__ void formant_gather(const float (&mag)[L / 64 + 1], const float (&phc)[L / 64 + 1],
                                               const float (&le)[L / 64 + 1], int multi, const int* srcl,
                                               float2* tile, int lane, float2 (&Y)[L / 64 + 1]) {
    constexpr int E = L / 64;
#pragma unroll
    for (int i = 0; i < E; ++i) tile[lane + 64 * i] = make_float2(mag[i] * exp_hw(-le[i]), phc[i]);
    {
        const bool l0 = lane == 0;
        tile[l0 ? L : L + 1] = make_float2(l0 ? mag[E] * exp_hw(-le[E]) : 0.0f, l0 ? phc[E] : 0.0f);
    }
    wave_lds_sync();
    i2v sc[E + 1];
    float2 f[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) sc[i] = lds_ld2i(&srcl[2 * ((i == E) ? L : lane + 64 * i)]);
#pragma unroll
    for (int i = 0; i <= E; ++i) f[i] = lds_ld(&tile[sc[i].x >= 0 ? sc[i].x : 0]);
    auto finish = [&](auto multi_tag) {
#pragma unroll
        for (int i = 0; i <= E; ++i) {
            const int sidx = sc[i].x;
            float ms = (sidx >= 0) ? f[i].x : 0.0f;
            const float pc = (sidx >= 0) ? f[i].y : 0.0f;
            if constexpr (decltype(multi_tag)::value)
                for (int qq = 1; qq < sc[i].y; ++qq) ms += lds_ld(&tile[sidx + qq]).x;
            ms *= exp_hw(le[i]);
            float sn, cs;
            sincos_rev(pc, &sn, &cs);
            Y[i] = make_float2(ms * cs, ms * sn);
        }
    };
    // (the ratio test is wave-uniform and hoisted, as in the plain gather)
    if (multi) finish(std::true_type{});
    else finish(std::false_type{});
}

}  // namespace pv
