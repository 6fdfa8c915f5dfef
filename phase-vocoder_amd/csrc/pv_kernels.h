// pv_kernels.h — kernel parameter blocks and launchers (host <-> device interface of libpv).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// Diagnostic builds.  The timing-only ablation switches (PV_ABL_*) give WRONG outputs and
// PV_FUSED_STAMPS writes per-wave clock stamps; a build that defines one must say so with
// PV_DIAGNOSTIC_BUILD, and the library then reports it (pv_diagnostic_build() = 1): bench.py
// refuses to check or report such a build as the product, and the GPU tests refuse it.
#if (defined(PV_ABL_NOSTORE) || defined(PV_ABL_NOATAN) || defined(PV_ABL_NOFFT) || defined(PV_ABL_NOWIN) ||   \
     defined(PV_ABL_L2IN) || defined(PV_ABL_L2ROWS) || defined(PV_ABL_NOSINCOS) || defined(PV_ABL_NOGATHER) || \
     defined(PV_FUSED_STAMPS)) &&                                                                            \
    !defined(PV_DIAGNOSTIC_BUILD)
#error "diagnostic / timing-only switch without PV_DIAGNOSTIC_BUILD (its outputs are wrong or instrumented)"
#endif

namespace pv {

// STANDARD run record per (channel, run): kRecFields rows of bins_pad int32 words —
// S = sum of the unwrap decisions of the run's frames after its first, then phi of the run's
// first and of its last frame (float bits).  k_carry makes the first frame's decision from
// phi(t0) and the previous run's last phase.
constexpr int kRecFields = 3;

struct AnaParams {
    const float* x;
    long long ldx, n;
    int hop, frames, F, nruns;
    int aligned;            // x base, ldx and hop allow 8-byte vector loads
    const float* win;       // analysis window (N)
    const float2* tw;       // stage-major twiddles of the L-point FFT (L entries)
    const float2* tws;      // real-split twiddles e^{-2 pi i k / (2L)}, k <= L
    const float* ek;        // expected advance (STANDARD), bins
    int ek_lane;            // 64 % hop_div == 0: e_k = ek[k mod 64] (per-lane constant)
    float2* spec;
    long long ld_spec;
    int spec_stride;
    int* runsum;            // [C][nruns][kRecFields][bins_pad] run records or nullptr
    int bins_pad;
    int nan_faithful;       // REF_COMPAT: x=y=0 -> NaN phase (kernel.cu:108)
    int packed;             // STANDARD rows in the PV_SPEC_PACKED layout (bin L in slot 0)
    int src_hi;             // STANDARD, L >= 1024: bins above it are not analysed (their row
                            // slots are not written; the synthesis does not read them:
                            // k_synthesis NR) — pv_process without a spectrum output; L
                            // otherwise
};

struct ScanParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, frames, F, nruns, L, bins_pad;
    int packed;                        // PV_SPEC_PACKED rows
    const float* ek;
    int* runsum;
    int* carry;
    // a segment of a longer stream (pv_segment_resynthesis), or nullptr: the unwrap count
    // before the segment's first frame and the phase of the frame before it, [C][bins_pad]
    const int* carry_in;
    const float* phi_in;
};

// per-segment summaries of a stream split into consecutive frame segments
// (pv_segment_summary / pv_segment_resynthesis): [seg][C][kSegFields][bins_pad] int32 —
// the segment's unwrap decisions after its first frame, phi of its first and of its last frame
constexpr int kSegFields = 3;
struct SegParams {
    const int* runsum;                 // the segment's run records (k_runsum)
    int nruns, L, bins_pad, channels;
    const float* ek;
    int* summary;                      // k_segsum: this segment's [C][kSegFields][bins_pad]
    const int* summaries;              // k_segcarry: the earlier segments' summaries
    int seg;                           // k_segcarry: how many segments come before this one
    int* carry_in;                     // k_segcarry outputs, [C][bins_pad]
    float* phi_in;
};

struct SynParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, frames, F, nruns, bins_pad;
    const int* carry;
    const float* ek;
    const unsigned* jk_mod;            // (p * j_k) mod q
    const int* src_first;              // pitch map
    const int* src_cnt;
    int pitch;
    float rho;
    unsigned long long p_mod, q;
    int q_pow2;
    float inv_q;
    const float2* tw;                  // stage-major twiddles, L-point
    const float2* tws;                 // e^{-2 pi i k/N}, k <= L
    const float* gain;                 // synthesis window * norm / N   (N)
    int rot;                           // 0 (STANDARD) or N/2 (REF_COMPAT swap halves)
    int hs;                            // out hop
    float* out;
    long long ldo, out_len;
    int out_aligned;                   // out base and ldo allow 8-byte vector stores
    float* tails;                      // [C][nwg][tail_len], nwg = ceil(nruns/4)
    int tail_len;
    int k_lane;                        // e_k, (p j_k) mod q depend on k mod 64 only (syn_run LANEK)
    int packed;                        // PV_SPEC_PACKED rows (bins 0 and L in slot 0)
    int src_hi;                        // highest analysis bin an output bin reads (single-
                                       // source pitch: the row slots above it are not read)
    unsigned t_off;                    // (index of the first frame in the whole stream) mod q:
                                       // 0 unless a segment of a longer stream
    // k_synthesis in the formant and warp modes (nullptr otherwise): the frames' log
    // envelope rows, env[c * ld_env + t * env_stride + k], k <= L (k_envelope)
    const float* env;
    long long ld_env;
    int env_stride;
    // k_synthesis in the reset modes (pv_transient.hip) has no pitch map and no envelope: its
    // arguments travel in those fields (reset_args below), so the block keeps its size and
    // layout and no other kernel's code changes
};

// The reset modes' view of SynParams: flags[c * ld_flags + t] != 0: frame t is a transient;
// theta[(c * nruns + run) * bins_pad + k]: Theta after the run's last flagged frame (k_reset;
// revolutions); prev_reset_run[c * nruns + run]: the last run below `run` that holds a flagged
// frame, or -1 (k_pick).
struct ResetArgs {
    const unsigned char* flags;
    long long ld_flags;
    const float* theta;
    const int* prev_reset_run;
};
__host__ __device__ inline ResetArgs reset_args(const SynParams& p) {
    return ResetArgs{reinterpret_cast<const unsigned char*>(p.src_cnt), p.ld_env, p.env, p.src_first};
}
inline void set_reset_args(SynParams* p, const ResetArgs& a) {
    p->src_cnt = reinterpret_cast<const int*>(a.flags);
    p->ld_env = a.ld_flags;
    p->env = a.theta;
    p->src_first = a.prev_reset_run;
}

// The time-map stretch (pv_timemap.hip).  Output frame u is built at analysis
// position i_u + a_u: map[u] = {i_u, a_u} (pv_timemap_split): one map for all channels, or one row
// of `ld_map` entries per channel (pv_timemap_set_channels).
struct MapEntry {
    int idx;
    float frac;
};
// The map modes' view of SynParams (no pitch map, no envelope; `frames`, F, nruns count output
// frames; `carry` is k_map_carry's, Phi at every run's first frame): the map and the number of
// analysed rows, every idx <= aframes - 1 (checked by the host).  Channel c reads map + c * ld_map
// (0: the shared map) and has counts[c] output frames (nullptr: `frames`); the frames from
// counts[c] on contribute nothing.
struct MapArgs {
    const MapEntry* map;
    int aframes;
    long long ld_map;
    const int* counts;
};
__host__ __device__ inline MapArgs map_args(const SynParams& p) {
    return MapArgs{reinterpret_cast<const MapEntry*>(p.src_first), p.env_stride, p.ld_env, p.src_cnt};
}
inline void set_map_args(SynParams* p, const MapArgs& a) {
    p->src_first = reinterpret_cast<const int*>(a.map);
    p->env_stride = a.aframes;
    p->ld_env = a.ld_map;
    p->src_cnt = a.counts;
}
// k_map_sum: sum[(c * nruns + r) * bins_pad + k] = the sum over run r's output frames u of
// Delta(i_u)[k] = P(i_u + 1)[k] - P(i_u)[k] (0 for i_u = aframes - 1), modulo 2^32;
// k_map_carry: carry[(c * nruns + r) * bins_pad + k] = P(i_0)[k] + the sums of the runs before r
struct MapScanParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, aframes;
    int frames, F, nruns;              // output frames (the map's length), per run, runs
    int L, bins_pad;
    int packed;                        // PV_SPEC_PACKED rows
    const MapEntry* map;
    long long ld_map;                  // entries between the channels' maps (0: one shared map)
    const int* counts;                 // output frames per channel (nullptr: `frames`)
    unsigned* sum;
    unsigned* carry;
};

// transient detector and reset offsets (pv_transient.hip)
// k_onset: dst[c * ld_dst + t] = {rise, tot} of frame t: rise = sum over bins 0 .. L of
// max(0, mag_t[k] - mag_{t-1}[k]) (mag_{-1} = 0), tot = sum of mag_t[k]; fp32, the kernel's order
struct OnsetParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, frames, F, nruns;
    int packed;                        // PV_SPEC_PACKED rows
    float2* dst;
    long long ld_dst;
};
// k_pick: flags from the strengths (strength != nullptr) — flag[t] = t >= 1 and rise[t] > thr
// tot[t] and rise[t] > rise[t-1] and rise[t] >= rise[t+1] (rise[frames] = 0) — and, from the
// flags, prev_reset_run
struct PickParams {
    const float2* strength;            // nullptr: the flags are the caller's, only the run scan
    long long ld_strength;
    float thr;
    unsigned char* flags;
    long long ld_flags;
    int* prev_reset_run;               // [C][nruns]
    int frames, F, nruns;
};
// k_reset: theta of every run that holds a flagged frame, from the run's carry and its rows up
// to its last flagged frame
struct ResetParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, frames, F, nruns, bins_pad;
    int packed;
    const int* carry;                  // nullptr: q = 1, no unwrap state
    const float* ek;
    const unsigned* jk_mod;
    float rho;
    unsigned long long p_mod, q;
    int q_pow2;
    float inv_q;
    const unsigned char* flags;
    long long ld_flags;
    float* theta;                      // [C][nruns][bins_pad]
};

// log spectral envelope of every frame (k_envelope, pv_formant.hip): the cepstrum of the
// frame's log magnitude, liftered to |quefrency| <= order, back in the log-spectrum domain
struct EnvParams {
    const float2* spec;
    long long ld_spec;
    int spec_stride, frames, F, nruns;
    int packed;                        // PV_SPEC_PACKED rows
    int order;                         // 1 .. N/4
    const float2* tw;                  // the v3 pass table of the L-point FFT (both directions)
    const float2* tws;                 // e^{-2 pi i k/N}, k <= L
    float* env;                        // env[c * ld_env + t * env_stride + k] = le[k], k <= L
    long long ld_env;
    int env_stride;
    int env_tail;                      // row slots written from L on: 1 (bin L), or 16 (bin L
                                       // and 15 zeros: the row store is whole 64-byte segments)
};

// single-launch STANDARD path for q = 1 (pv_fused.hip)
struct FusedParams {
    const float* x;
    long long ldx, n;
    int hop, frames, F, nruns;
    int aligned;                       // x base, ldx and hop allow 8-byte vector loads
    const float* win;                  // analysis window (N)
    const float2* tw;                  // stage-major twiddles, L-point (analysis = synthesis)
    const float2* tws;                 // e^{-2 pi i k/N}, k <= L
    const int* src_first;              // pitch map
    const int* src_cnt;
    float rho;
    const float* gain;                 // synthesis window * norm / N   (N)
    const float2* tw_half;             // stage-major L/2-point table (pitch 2: MODE 4) or nullptr
    int hs;                            // out hop
    float2* spec;
    long long ld_spec;
    int spec_stride;
    float* out;
    long long ldo, out_len;
    int out_aligned;
    float* tails;                      // [C][nwg][tail_len], nwg = ceil(nruns/4)
    int tail_len;
    int* seam_flags;                   // [C][nwg] arrival counters, 0 between launches
    int packed;                        // PV_SPEC_PACKED rows
    int src_hi;                        // highest analysis bin an output bin reads (pitch > 1:
                                       // about L / pitch): with spec == nullptr the bins above
                                       // it are not analysed (nothing reads their phase)
    int nwg;                           // workgroups per channel (grid.x)
    int n4;                            // > 0: balanced runs — n4 of them have F + 1 frames
                                       // (k_fused: which ones, so that no SIMD holds more than
                                       // two of them); 0: every run F frames
#ifdef PV_FUSED_STAMPS
    unsigned long long* stamps;        // diagnostic build only: kFusedStampSlots per wave
#endif
};
#ifdef PV_FUSED_STAMPS
constexpr int kFusedStampSlots = 16;  // rt start, mt start, setup, frame 0..F-1, loop, end rt/mt, hw id
#endif

// channel-resident STANDARD time stretch (pv_resident.hip): one workgroup per channel, the
// spectrum rows stay in LDS
struct ResidentParams {
    const float* x;
    long long ldx, n;
    int hop, frames, F;                // F: the handle's frames per run (the split path's seams)
    const float* win;                  // analysis window (N)
    const float2* tw;                  // stage-major twiddles, L-point (analysis = synthesis)
    const float2* tws;                 // e^{-2 pi i k/N}, k <= L
    const float* ek;                   // per-lane unwrap constants: e_k, (p j_k) mod q
    const unsigned* jk_mod;
    float rho, inv_q;
    unsigned p_mod, q;                 // q a power of two <= 4096
    const float* gain;                 // synthesis window * norm / N   (N)
    int hs;                            // out hop
    float* out;
    long long ldo, out_len;
};

struct SeamParams {
    float* out;
    long long ldo, out_len;
    const float* tails;
    const float* ola_in;
    long long ld_ola;
    int nruns, nwg, F, hs, tail_len;
};

// real-time mode (pv_rt.hip): one launch per callback, a wave per channel
struct RtParams {
    const float* in;                   // [C][nframes * hop] new samples (row stride ldi)
    long long ldi;
    float* out;                        // [C][nframes * hs] emitted samples (row stride ldo)
    long long ldo;
    float2* spec;                      // optional [C][nframes][spec_stride] {mag, phase}
    long long ld_spec;
    int spec_stride;
    int channels, nframes, hop, hs, bins_pad;
    float* hist;                       // [C][N] stream state (see pv_rt.hip)
    float* ola;                        // [C][N]
    float* phprev;                     // [C][bins_pad]
    int* M;                            // [C][bins_pad]
    unsigned* tcount;                  // [C]
    const float* win;
    const float* gain;
    const float2* tw;
    const float2* tws;
    const float* ek;
    const unsigned* jk_mod;
    const int* src_first;
    const int* src_cnt;
    float rho;
    unsigned long long p_mod, q;
    int q_pow2;
    float inv_q;
};

// streaming resampler of the real-time pitch shift (pv_rt_pitch.hip): one launch per callback
// after k_rt, a workgroup per channel.  row[c * ld_row ..]: [H history | n_new stretched samples]
// (k_rt wrote the new ones at row + H); output u < n_out reads the 2W samples from
// row[H - 2W + 1 + (u P + off) / Q] on with the coefficients tab[((u P + off) mod Q) * 2W ..],
// then the last H samples of the row move to its front.
struct RtResampleParams {
    float* row;
    long long ld_row;
    float* out;                        // [C][n_out] (row stride ldo)
    long long ldo;
    const float* tab;                  // [Q][2W], c[r][t] = h(t - W + 1 - r / Q)
    int channels;
    int n_new, n_out;                  // nframes * out hop, nframes * hop
    int P, Q, W, H;
    unsigned off;                      // W Q - D P >= 0; (n_out - 1) P + off < 2^31
};

// real-time pitch map (pv_rt_pitchmap.hip): two launches per callback.  Per
// channel the stream keeps RtMapState (all zero at a stream's start; every position is relative to
// the scratch row, every counter saturates: nothing grows with the stream), a ring of the steps
// d_b whose blocks are not yet emitted, oldest first, and the scratch row
//   row[0 .. K)           the K >= W_max final stretched samples below row[K]'s position
//   row[K .. K + fill)    the final stretched samples from there on
// (S[n] = 0 for n < 0 is the zeroed row of a stream's start).
struct RtMapState {
    long long off;   // the next stretched frame's offset inside the current span, 2^-32 samples
    long long rpos;  // start of the next output block relative to row[K], 2^-32 samples (< 2^32
                     // between callbacks)
    int rows;        // 0: the next analysed row is the stream's first; 1 otherwise
    int fill;        // see above
    int nsteps;      // steps waiting in the ring
    int emitted;     // output blocks emitted, saturating at G + 1 (the first G + 1 are zeros)
};
// k_rt_map: k_rt's analysis (rt: its block; out, ldo, hs, phprev, M, tcount and the unwrap and
// pitch tables are not used), then per pushed frame the stretched frames of the span that frame
// closes, appended to the row; the frame's step goes into the ring.
struct RtMapParams {
    RtParams rt;
    const float* ratio;                // [C][nframes] (row stride ldr), or nullptr: 1
    long long ldr;
    float ratio_min, ratio_max;
    float2* prev;                      // [C][bins_pad] {mag, bits of P} of the last analysed row
    unsigned* phi;                     // [C][bins_pad] Phi, fractions of a turn
    RtMapState* st;                    // [C]
    long long* ring;                   // [C][ring_cap]
    int ring_cap;                      // >= G + the largest nframes
    float* row;                        // [C][ld_row]
    long long ld_row;
    int K;
};
// k_rt_varresample: nframes output blocks of hop samples per channel from the row, then the row's
// unread tail moves to its front.  The host has sized the row and the ring
// (pvtab::rt_pitchmap_plan): neither kernel checks anything.
struct RtVarParams {
    float* row;
    long long ld_row;
    int K;
    float* out;                        // [C][nframes * hop] (row stride ldo)
    long long ldo;
    RtMapState* st;
    long long* ring;
    int ring_cap;
    const float2* win;                 // the window table of pv_varresample.hpp
    float win_scale;
    int channels, nframes, hop, G;
    double rolloff, Z;                 // the preset's (Sq_b and W_b are computed here, in fp64)
};

// real-time harmoniser (pv_rt_harmon.hip): V voices of the real-time pitch map per
// channel, two launches per callback.  Per (channel, voice) — index c V + v — the stream keeps what
// the pitch map keeps per channel (RtMapState, Phi, the overlap accumulator, the scratch row), a
// ring of {step, gain} of the blocks not yet emitted, and the gain of the last emitted block; per
// channel the input history and the last analysed row.
constexpr int kRtHarmonMaxVoices = 8;
struct RtHStep {
    long long d;     // the block's step, 2^-32 samples
    float gain;      // the block's gain (a NaN stored as 0)
    int pad;
};
struct RtHGain {
    float g;         // gain of the last emitted block
    int have;        // 0: no block emitted yet (block 0 ramps from its own gain)
};
// k_rt_hmap: RtMapParams with a voice dimension (rt.ola is not used: the accumulators are ola)
struct RtHMapParams {
    RtParams rt;
    int voices;
    const float* ratio;                // [C][V][nframes] (row stride ld_ctl), or nullptr: 1
    const float* gain;                 // [C][V][nframes] (row stride ld_ctl), or nullptr: 1 / V
    long long ld_ctl;
    float ratio_min, ratio_max;
    float2* prev;                      // [C][bins_pad] {mag, bits of P} of the last analysed row
    unsigned* phi;                     // [C][V][bins_pad] Phi, fractions of a turn
    float* ola;                        // [C][V][N] overlap accumulators
    RtMapState* st;                    // [C][V]
    RtHStep* ring;                     // [C][V][ring_cap]
    int ring_cap;                      // >= G + the largest nframes
    float* row;                        // [C][V][ld_row]
    long long ld_row;
    int K;
};
// k_rt_hresample: RtVarParams with a voice dimension and the mix
struct RtHVarParams {
    float* row;
    long long ld_row;
    int K;
    float* mix;                        // [C][nframes * hop] (row stride ldo)
    long long ldo;
    float* voices_out;                 // [V][C][nframes * hop] (row stride ld_voice), or nullptr
    long long ld_voice;
    RtMapState* st;
    RtHStep* ring;
    int ring_cap;
    RtHGain* gprev;                    // [C][V]
    const float2* win;                 // the window table of pv_varresample.hpp
    float win_scale;
    int channels, voices, nframes, hop, G;
    double rolloff, Z;                 // the preset's (Sq_b and W_b are computed here, in fp64)
};

// harmoniser mix: dst[c][i] = sum_k gain[k] * src[k][c][i]
struct MixParams {
    const float* src;
    long long ldo, ld_voice;
    int voices;
    float gain[64];
    float* dst;
    long long ld_mix, len;
    int channels;
};

hipError_t launch_std_analysis(int L, int channels, const AnaParams& p, hipStream_t s);
int std_analysis_wgs_per_cu(int L, int hop, bool ek_lane, bool packed, int* waves_per_wg);
hipError_t launch_compat_analysis(int L, int channels, const AnaParams& p, hipStream_t s);
hipError_t launch_runsum(int channels, const ScanParams& p, hipStream_t s);
hipError_t launch_carry(int channels, const ScanParams& p, hipStream_t s);
hipError_t launch_segsum(const SegParams& p, hipStream_t s);
hipError_t launch_segcarry(const SegParams& p, hipStream_t s);
hipError_t launch_synthesis(int L, int mode, int channels, const SynParams& p, hipStream_t s);
// STANDARD time stretch with identity phase locking (pv_locked.hip): launch_synthesis's mode 0
// with every bin's output phase taken from the magnitude peak that owns it; same SynParams
// (k_lane and src_hi are not used), same tails for launch_seam
hipError_t launch_synthesis_locked(int L, int channels, const SynParams& p, hipStream_t s);
// formant-preserving STANDARD pitch shift (pv_formant.hip): the envelope rows, then
// launch_synthesis's mode 2 with the formant gather (SynParams.env; k_lane and src_hi are not
// used), same tails for launch_seam.  L <= 1024.
hipError_t launch_envelope(int L, int channels, const EnvParams& p, hipStream_t s);
hipError_t launch_synthesis_formant(int L, int channels, const SynParams& p, hipStream_t s);
// STANDARD time stretch with the envelope warp (pv_warp.hip; pv_pitch_set_formant): launch_synthesis's
// mode 0, or launch_synthesis_locked with lock != 0, with every magnitude scaled by the frame's
// envelope at the bin's warp position.  SynParams.env: the rows launch_envelope wrote;
// src_first / src_cnt carry the warp map {i_k} / {bits of f_k}, k <= L (a time stretch has no
// pitch map; k_lane and src_hi are not used); same tails for launch_seam.  L <= 1024.
hipError_t launch_synthesis_warp(int L, int lock, int channels, const SynParams& p, hipStream_t s);
// STANDARD time stretch with the transient phase reset (pv_transient.hip; pv_set_transient):
// launch_synthesis's mode 0, or launch_synthesis_locked with lock != 0, with Theta added to every
// output phase (set_reset_args; k_lane and src_hi are not used); same
// tails for launch_seam.  L <= 1024.  Before it: launch_onset and launch_pick (or launch_pick
// alone on the caller's flags), the carries, launch_reset.
hipError_t launch_onset(int L, int channels, const OnsetParams& p, hipStream_t s);
hipError_t launch_pick(int channels, const PickParams& p, hipStream_t s);
hipError_t launch_reset(int L, int channels, const ResetParams& p, hipStream_t s);
hipError_t launch_synthesis_reset(int L, int lock, int channels, const SynParams& p, hipStream_t s);
// The time-map stretch (pv_timemap.hip; pv_timemap_process): launch_map_sum, launch_map_carry,
// then launch_synthesis's mode 0, or launch_synthesis_locked with lock != 0, at out hop = hop with
// the map's phases and magnitudes (set_map_args; ek, jk_mod, k_lane and src_hi are not used);
// register overlap-add at hop 128 / 256 / 512, the LDS ring otherwise; same tails for
// launch_seam.  L <= 1024.
hipError_t launch_map_sum(int channels, const MapScanParams& p, hipStream_t s);
hipError_t launch_map_carry(int channels, const MapScanParams& p, hipStream_t s);
hipError_t launch_synthesis_map(int L, int lock, int channels, const SynParams& p, hipStream_t s);
// the synthesis kernel for this geometry can take SynParams.k_lane (register overlap-add,
// power-of-two q, STANDARD)
bool synthesis_lane_kernel(int L, int mode, int hs, bool q_pow2, unsigned long long q);
hipError_t launch_seam(int channels, const SeamParams& p, hipStream_t s);
bool fused_supported(int L, int hs);
hipError_t launch_fused(int L, int mode, int channels, const FusedParams& p, hipStream_t s);
// the channel-resident kernel exists for this geometry (the host predicate
// pvtab::resident_supported admits no other), and its launch
bool resident_kernel(int L, int hs);
hipError_t launch_resident(int L, int channels, const ResidentParams& p, hipStream_t s);
size_t synthesis_lds_bytes(int L, int hs);
hipError_t launch_fft(int n, int inverse, const float2* in, float2* out, const float2* tw, int batch,
                      hipStream_t s);
hipError_t launch_mix(const MixParams& p, hipStream_t s);
// mode: 0 STANDARD stretch, 2 STANDARD pitch, kRtModeLocked the stretch with identity phase locking
constexpr int kRtModeLocked = 6;  // (= kModeLocked, pv_lock.hpp)
hipError_t launch_rt(int L, int mode, const RtParams& p, hipStream_t s);
size_t rt_lds_bytes(int L);
hipError_t launch_rt_resample(const RtResampleParams& p, hipStream_t s);
// real-time pitch map (pv_rt_pitchmap.hip): the geometries k_rt_map is built for, and the launches
bool rt_map_kernel(int L);
hipError_t launch_rt_map(int L, int lock, const RtMapParams& p, hipStream_t s);
hipError_t launch_rt_varresample(const RtVarParams& p, hipStream_t s);
// real-time harmoniser (pv_rt_harmon.hip): the most voices k_rt_hmap takes at this size (0: no
// kernel), and the launches
int rt_hmap_max_voices(int L);
hipError_t launch_rt_hmap(int L, int lock, const RtHMapParams& p, hipStream_t s);
hipError_t launch_rt_hresample(const RtHVarParams& p, hipStream_t s);
hipError_t launch_window_gain(const float* win, float* dwin, float* gain, int n, hipStream_t s);
hipError_t launch_overlap_test(const float* in, const float* win, const float* back, float* out,
                               int n, int hop, hipStream_t s);

}  // namespace pv
