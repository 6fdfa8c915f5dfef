// pv_timemap.hip — the time-map stretch (pv_timemap_process): the integer
// phase scan over the map (k_map_sum, k_map_carry) and the instantiations of k_synthesis
// (pv_syn_kernel.hpp) in the map modes.
//
//   k_map_sum     per (channel, run of F output frames): the sum of the phase steps Delta(i_u)
//   k_map_carry   per (channel, bin): Phi at every run's first frame, P(i_0) + the earlier sums
//   k_synthesis<kModeMap / kModeLockedMap>   two rows per frame, Phi in registers
// All sums are uint32 (fractions of a turn, modulo 2^32): exact and associative, so the result
// does not depend on the run length.  Nothing waits on another workgroup, nothing allocates or
// synchronises: all capturable.  Every row index (i_u, i_u + 1 <= aframes - 1) and every run
// and carry row is in range by the host's checks (pv_timemap_set, pv_timemap_process).
// Channel c reads the map at map + c * ld_map (0: one map for all channels) and has counts[c]
// output frames (nullptr: `frames`; pv_timemap_set_channels): a run past a
// channel's count sums nothing and synthesises zeros.
#include "pv_syn_kernel.hpp"

namespace pv {

// ------------------------------------------------------------------ k_map_sum
// One wave = one run, 4 runs per workgroup.  The lane holds P of bins lane + 64 i (i < E) and
// lane 0 that of bin L (slot E).  The map entry is wave-uniform (scalar reads).  A frame at the
// last analysed row adds nothing (Delta(aframes - 1) = 0) and loads nothing; a frame whose lower
// row is the previous frame's upper row keeps it in registers (a map near rate 1).
template <int L>
__global__ __launch_bounds__(256) void k_map_sum(MapScanParams p) {
    constexpr int E = L / 64;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.y;
    const int run = blockIdx.x * 4 + w;
    if (run >= p.nruns) return;
    const int t0 = run * p.F;
    const int frames_c = p.counts ? __builtin_amdgcn_readfirstlane(p.counts[c]) : p.frames;
    const int nfr = max(0, min(p.F, frames_c - t0));
    const MapEntry* mapc = p.map + (long long)c * p.ld_map + t0;
    const float2* specc = p.spec + (long long)c * p.ld_spec;
    const bool packed = p.packed != 0;
    auto load = [&](int t, unsigned (&P)[E + 1]) {
        const float2* row = specc + (long long)t * p.spec_stride;
        float2 sv[E + 1];
        PV_FOR_BINS(E, lane, {
            if (i < E || !packed) sv[i] = row[k];
        })
        if (packed && lane == 0) unpack_real_bins(sv[0], sv[0], sv[E]);
        PV_FOR_BINS(E, lane, { P[i] = phase_turns(sv[i].y); })
    };
    const int alast = p.aframes - 1;
    unsigned S[E + 1], P0[E + 1], P1[E + 1];
#pragma unroll
    for (int i = 0; i <= E; ++i) S[i] = P1[i] = 0u;
    int held = -1;  // the row P1 holds (wave-uniform)
    for (int u = 0; u < nfr; ++u) {
        const int iu = __builtin_amdgcn_readfirstlane(mapc[u].idx);
        if (iu >= alast) continue;
        if (held == iu) {
#pragma unroll
            for (int i = 0; i <= E; ++i) P0[i] = P1[i];
        } else {
            load(iu, P0);
        }
        load(iu + 1, P1);
        held = iu + 1;
        PV_FOR_BINS(E, lane, { S[i] += P1[i] - P0[i]; })
    }
    unsigned* dst = p.sum + ((long long)c * p.nruns + run) * p.bins_pad;
    PV_FOR_BINS(E, lane, { dst[k] = S[i]; })
}

// ------------------------------------------------------------------ k_map_carry
// One thread per (channel, bin): an exclusive scan of the run sums from P(i_0), four runs' loads
// in flight at a time (k_carry's shape without its unwrap decisions).
__global__ __launch_bounds__(64) void k_map_carry(MapScanParams p) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    const int c = blockIdx.y;
    if (k > p.L) return;
    const int BP = p.bins_pad;
    // PV_SPEC_PACKED rows: bins 0 and L are the sign bits of slot 0 {s0, sL}
    const bool real_bin = p.packed && (k == 0 || k == p.L);
    const int i0 = p.map[(long long)c * p.ld_map].idx;
    const float2 v = p.spec[(long long)c * p.ld_spec + (long long)i0 * p.spec_stride + (real_bin ? 0 : k)];
    const float phi = !real_bin ? v.y : (__float_as_uint(k == 0 ? v.x : v.y) >> 31) ? kPi : 0.0f;
    unsigned M = phase_turns(phi);
    const unsigned* sm = p.sum + (long long)c * p.nruns * BP + k;
    unsigned* cr = p.carry + (long long)c * p.nruns * BP + k;
    int run = 0;
    for (; run + 4 <= p.nruns; run += 4) {
        unsigned sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[j] = sm[(long long)(run + j) * BP];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cr[(long long)(run + j) * BP] = M;
            M += sv[j];
        }
    }
    for (; run < p.nruns; ++run) {
        cr[(long long)run * BP] = M;
        M += sm[(long long)run * BP];
    }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_map_sum(int channels, const MapScanParams& p, hipStream_t s) {
    dim3 grid((p.nruns + 3) / 4, channels);
    switch (p.L) {
        case 128: hipLaunchKernelGGL(k_map_sum<128>, grid, dim3(256), 0, s, p); break;
        case 256: hipLaunchKernelGGL(k_map_sum<256>, grid, dim3(256), 0, s, p); break;
        case 512: hipLaunchKernelGGL(k_map_sum<512>, grid, dim3(256), 0, s, p); break;
        case 1024: hipLaunchKernelGGL(k_map_sum<1024>, grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_map_carry(int channels, const MapScanParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_map_carry, dim3((p.L + 1 + 63) / 64, channels), dim3(64), 0, s, p);
    return hipGetLastError();
}

// the kernel of launch_synthesis_locked for the same geometry at q = 1 (launch_syn_plain: register
// overlap-add at out hop 128 / 256 / 512), up to L = 1024
hipError_t launch_synthesis_map(int L, int lock, int channels, const SynParams& p, hipStream_t s) {
    const MapArgs ma = map_args(p);
    if (!ma.map || ma.aframes < 1 || !p.carry || p.q != 1ull) return hipErrorInvalidValue;
    dim3 grid((p.nruns + 3) / 4, channels);
    const int dt = syn_dt(L, p.hs);
    return lock ? launch_syn_plain<kModeLockedMap, true, 1024>(L, dt, grid, p, s)
                : launch_syn_plain<kModeMap, true, 1024>(L, dt, grid, p, s);
}

}  // namespace pv
