/*
 * pv.h — C-ABI of the MI355X phase-vocoder hot path (libpv.so).
 *
 * Plain pointers and sizes only; every float / pv_float2 pointer handed to a compute
 * entry point is a DEVICE pointer (hipMalloc / torch CUDA tensor) on the handle's device,
 * and `stream` is a hipStream_t (NULL = the legacy default stream).  All calls are
 * asynchronous with respect to the host (graph-capturable: no allocation, no sync) — the
 * one exception is pv_process(spec = NULL) on the split path, whose first call allocates
 * the handle's own rows unless pv_reserve_spectrum did (under capture it refuses instead).
 *
 * Which reference interface each entry point replaces (reference @ /root/reference):
 *   pv_create        PhaseVocoder(int samples, Effect e, float scale, int hop)
 *                      src/phaseVocoder.h:79-116  (window imp[], hop = samples/hop,
 *                      outHopSize = scale*hop, cuFFT plans, streams)
 *   pv_destroy       ~PhaseVocoder()  src/phaseVocoder.h:128-130; cufftDestroy main.cpp:396
 *   pv_analysis      PhaseVocoder::analysis_CUFFT  src/phaseVocoder.cpp:25-33
 *                      -> CudaPhase::pv_analysis_CUFFT  karnel/kernel.cu:299-348
 *                      batched over channels x frames (main.cpp:228-250 loop)
 *   pv_resynthesis   PhaseVocoder::resynthesis_CUFFT  src/phaseVocoder.cpp:60-76
 *                      -> CudaPhase::resynthesis_CUFFT  karnel/kernel.cu:352-432
 *                      batched, including the running overlap-add main.cpp:261-297
 *   pv_process       analysis -> processing -> resynthesis fused pipeline (the offline
 *                      loop of main.cpp:228-297 in one call); no reference counterpart
 *   pv_frame_*       the hop/frame arithmetic of main.cpp:231 and main.cpp:266
 *   pv_rt_*          the real-time design: RtAudio `callback` (main.cpp:45-59) copying each
 *                      buffer into PhaseVocoder::curr_input and calling the per-callback
 *                      PhaseVocoder::analysis() over prev_input / prev_mag_phase /
 *                      prev_output (phaseVocoder.h:16-31; pv_analysis_RT kernel.cu:219-250;
 *                      README.md:46-50); one hipGraph replay per callback
 *   pv_segment_*     one long stream split into consecutive frame segments, e.g. one per
 *                      GPU (the optional time shard); no reference
 *                      counterpart (the reference processes one stream frame by frame)
 *   pv_harmon*       the harmoniser the README plans ("multiple pitch shifts on a single
 *                      input", README.md:50): one analysis, K pitch-shift resyntheses
 *   pv_fft_c2c       FFT::HPFFT::computeGPUFFT / computeGPUIFFT (karnel/hpfft.h:6-11,
 *                      hpfft.cu:145-203): radix-2 Stockham FFT, batched in one launch
 *
 * Errors: status codes instead of the reference's print-and-exit (io.cpp:115-124).  The
 * header-only C++ drop-in (include/phaseVocoder.h) restores print-and-exit on top.
 *
 * Environment overrides (read by pv_create / pv_rt_capture; the tests use them to reach
 * every kernel geometry; none changes a result beyond run-boundary roundings):
 *   PV_RUN_FRAMES=F      frames per wave run of the split path (even, 8..256)
 *   PV_SYN_LANEK=0       per-bin unwrap constants from LDS instead of per-lane registers
 *   PV_FUSED=0           the split path even where the q = 1 single launch applies
 *   PV_FUSED_FRAMES=F    frames per run of the q = 1 single launch
 *   PV_FUSED_HALF=0      pitch 2 single launch: the MODE 3 gather and full-size inverse FFT
 *                        instead of the half-size resynthesis of X^2/|X| (MODE 4)
 *   PV_FUSED_BALANCE=0   single launch of one channel: uniform runs (no balanced F+1 runs)
 *   PV_RESIDENT=0|1      pv_process(spec = NULL) of a plain STANDARD stretch at N = 1024, hop
 *                        N/4, out hop 128: 0 never takes the channel-resident launch, 1 takes
 *                        it at any channel count; unset: from pv_resident_min_channels up
 *                        to 1024 channels (same output bits either way)
 *   PV_COMPAT_ANA_FRAMES=F  REF_COMPAT analysis run length (1..256, default 4)
 *   PV_RT_LAUNCH=direct  pv_rt_callback launches the kernel instead of replaying the graph
 *
 * Concurrency: a handle's compute calls share its workspace (run records, carries, seam
 * tails, segment state), so the calls on one handle must be ordered — one stream, or
 * streams synchronised between calls; different handles are independent.  pv_last_error
 * is per thread; pv_reserve_spectrum is thread-safe.
 */
#ifndef PV_H
#define PV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PV_ABI_VERSION 5  /* 2: pv_config.window / nan_faithful, pv_set_window;
                             3: pv_info.single_launch / single_launch_frames / lane_constants;
                             4: leading abi_version in pv_config / pv_info (checked: a caller
                                built against another header gets PV_ERR_ARG, not a
                                misread struct), pv_config.spec_layout, the chained path
                                and pv_check_device removed;
                             5: pv_config.tables_external, pv_process(spec = NULL) on the
                                single launch (later additions are functions only, no
                                struct change: pv_sources_sha, pv_reserve_spectrum,
                                pv_segment_*, pv_set_phase_lock / pv_get_phase_lock,
                                pv_set_formant / pv_get_formant, pv_spectral_envelope,
                                pv_harmonizer_set_formant, pv_resampler_* / pv_resample /
                                pv_resample_length, pv_pitch_reserve / pv_pitch_process /
                                pv_pitch_output_length, pv_rt_set_phase_lock /
                                pv_rt_get_phase_lock, pv_rt_pitch_reserve / pv_rt_pitch_latency /
                                pv_rt_pitch_push, pv_pitch_set_formant / pv_pitch_get_formant,
                                pv_varresampler_* / pv_varresample / pv_varresample_steps /
                                pv_varresample_length, pv_pitchmap_plan / pv_pitchmap_set /
                                pv_pitchmap_output_length / pv_pitchmap_process,
                                pv_resident_min_channels, pv_pitch_track / pv_pitch_correct_plan,
                                pv_timemap_set_channels / pv_timemap_channels,
                                pv_varresampler_set_maps / pv_varresample_map_channels,
                                pv_pitchmap_set_channels, pv_rt_pitchmap_reserve /
                                pv_rt_pitchmap_latency / pv_rt_pitchmap_push /
                                pv_rt_pitchmap_host_ratios) */

typedef struct pv_handle pv_handle;

/* layout-compatible with HIP/CUDA float2 {x, y} (8 bytes, 8-byte aligned) */
typedef struct pv_float2 {
    float x, y;
} pv_float2;

typedef enum pv_status {
    PV_OK = 0,
    PV_ERR_ARG = 1,         /* invalid argument / size out of the handle's capacity */
    PV_ERR_UNSUPPORTED = 2, /* configuration not supported (e.g. N not a power of 2) */
    PV_ERR_HIP = 3,         /* HIP runtime error (pv_last_error() has the text)       */
    PV_ERR_NOMEM = 4        /* device allocation failed                               */
} pv_status;

typedef enum pv_effect {
    PV_TIME_SHIFT = 't',  /* phaseVocoder.h:6  */
    PV_PITCH_SHIFT = 'p'  /* phaseVocoder.h:7  */
} pv_effect;

typedef enum pv_mode {
    PV_MODE_REF_COMPAT = 0, /* the reference's active path, bugs included */
    PV_MODE_STANDARD = 1    /* textbook phase vocoder (Hann, unwrap, true frequency)     */
} pv_mode;

/* STANDARD spectrum row layout (pv_config.spec_layout) */
typedef enum pv_spec_layout {
    PV_SPEC_NATURAL = 0, /* {mag, phase} of bins k = 0 .. N/2 (spec_bins = N/2+1), rows padded
                            to spec_stride = N/2 + 8                                          */
    PV_SPEC_PACKED = 1   /* rows of exactly N/2 float2 (spec_stride = spec_bins = N/2): bins
                            1 .. N/2-1 as {mag, phase}; bin 0 and bin N/2, both real, share
                            slot 0 as {s0, sN/2} with s = +mag for phase 0, -mag for phase pi
                            (the sign bit carries the phase; pv_unpack_bins below).  Every
                            row store is whole 64-byte segments (no 8-byte partial write for
                            bin N/2).  STANDARD handles only; the real-time mode rejects it */
} pv_spec_layout;

typedef enum pv_window {
    PV_WINDOW_DEFAULT = 0,     /* the mode's window: REF_COMPAT the symmetric Hamming of the
                                  4-argument constructor, STANDARD the periodic Hann        */
    PV_WINDOW_HAMMING_REF = 1, /* 0.54f - 0.46f*cosf(w*i), w = (float)(2pi/(N-1))
                                  (src/phaseVocoder.h:85-89; REF_COMPAT)                    */
    PV_WINDOW_HANN_REF = 2     /* 0.5f*(1.f - cosf((float)(2pi*i/N))) of the 1-argument
                                  constructor (src/phaseVocoder.h:64-66; REF_COMPAT)        */
} pv_window;

typedef struct pv_config {
    int abi_version;  /* = PV_ABI_VERSION (pv_create rejects any other value)          */
    int n_samps;      /* N, window length: power of 2 in [256, 2048] (both modes)       */
    int hop_div;      /* hop = N / hop_div (phaseVocoder.h:79 4th argument is a divisor)  */
    int effect;       /* pv_effect                                                      */
    float scale;      /* TIME_SHIFT: out_hop = (int)(scale*hop); PITCH_SHIFT: pitch ratio */
    int mode;         /* pv_mode                                                        */
    int max_channels; /* workspace capacity                                             */
    int max_frames;   /* workspace capacity, frames per channel                          */
    int device;       /* HIP device ordinal                                             */
    int window;       /* pv_window (0 = the mode's default); STANDARD accepts only 0      */
    int nan_faithful; /* REF_COMPAT: a bin with Re = Im = 0 gets phase atanf(0/0) = NaN as
                         in the reference (kernel.cu:101-109), which poisons that frame's
                         resynthesis; 0 (default) gives phase 0 (SURVEY.md §8c deviation 4) */
    int spec_layout;  /* pv_spec_layout (STANDARD only; REF_COMPAT accepts 0)              */
    int tables_external; /* 1: the handle's constant tables (windows, gains, twiddles, unwrap
                            and pitch maps) are not built here — the device tables start
                            zeroed and every compute call returns PV_ERR_ARG until
                            pv_import_tables loads a blob (a non-root rank of a multi-GPU
                            job receives rank 0's over RCCL, pvamd.dist.broadcast_tables);
                            0 (default): built by pv_create.  Batch handles only (pv_rt /
                            harmoniser reject it) */
} pv_config;

typedef struct pv_info {
    int abi_version;    /* the caller sets PV_ABI_VERSION (pv_get_info checks it)           */
    int n_samps, hop, out_hop;
    int spec_bins;      /* slots written per frame: N/2+1 (STANDARD natural), N/2 (STANDARD
                           packed) or 2N (REF_COMPAT)                                     */
    int spec_stride;    /* pv_float2 elements between consecutive frames of a channel   */
    int frames_per_run; /* frames per wave run; chosen from           */
                        /* max_channels x max_frames, or the environment variable       */
                        /* PV_RUN_FRAMES (even, 8..256) read by pv_create               */
    int mode, effect;
    float scale;
    int single_launch;        /* what pv_process launches: 0 the split path (analysis, scan,
                                 synthesis, seams), 1 one q = 1 launch (pv_fused.hip)      */
    int single_launch_frames; /* frames per run of that launch (0 for the split path)     */
    int lane_constants;       /* 1: the split synthesis keeps the per-bin unwrap constants
                                 in registers (e_k and (p j_k) mod q repeat every 64 bins:
                                 64 a multiple of N / hop and q of 64 hop / N, e.g. config
                                 3 and 4); PV_SYN_LANEK=0 read by pv_create turns it off  */
    int spec_layout;          /* pv_spec_layout of the handle's spectrum rows               */
} pv_info;

/* A PV_SPEC_PACKED row's slot 0 -> {mag, phase} of bin 0 and bin N/2.  Exact: the packed
 * phases are +0 or the float nearest pi (0x1.921fb6p+1f) and the magnitude is the sign-free
 * slot value. */
static inline void pv_unpack_bins(pv_float2 slot0, pv_float2* bin0, pv_float2* bin_half) {
    const float pi = 0x1.921fb6p+1f;
    union { float f; unsigned u; } a, b;
    a.f = slot0.x;
    b.f = slot0.y;
    const unsigned sa = a.u >> 31, sb = b.u >> 31;
    a.u &= 0x7fffffffu;
    b.u &= 0x7fffffffu;
    bin0->x = a.f;
    bin0->y = sa ? pi : 0.0f;
    bin_half->x = b.f;
    bin_half->y = sb ? pi : 0.0f;
}

int pv_abi_version(void);
/* version of the fp32 PV_STANDARD analysis contract (the exact operation sequence of the
 * phases and unwrap decisions) this build computes; the CPU oracle states the
 * version it restates (oracle/pvref.h PVR_CONTRACT_VERSION) and the two must agree */
int pv_contract_version(void);
/* 1 for a diagnostic build (timing-only ablations or instrumentation compiled in with
 * PV_DIAGNOSTIC_BUILD: outputs are not the product's), 0 for the product */
int pv_diagnostic_build(void);
/* sha256[:16] of the sources this library was built from (phase-vocoder_amd/csrc: every
 * *.hip *.hpp *.h *.cpp and the Makefile in byte order, then include/pv.h), compiled in by the
 * Makefile: the Python binding refuses a library whose hash is not its tree's */
const char* pv_sources_sha(void);
const char* pv_status_string(pv_status s);
const char* pv_last_error(void); /* thread-local text of the last failure */

pv_status pv_create(const pv_config* cfg, pv_handle** out);
void pv_destroy(pv_handle* h);
pv_status pv_get_info(const pv_handle* h, pv_info* info);

/* main.cpp:231 — analysis frames of an n-sample channel: ceil((n - hop)/hop), >= 0 */
int pv_frame_count(long long n_samples, int hop);
/* samples of the full overlap-add of `frames` frames: frames*out_hop + N - out_hop */
long long pv_output_length(const pv_handle* h, int frames);

/* Analysis of `frames` frames per channel.  Frame t of channel c reads
 * x[c*ldx + t*hop + i], i < N; samples at index >= n_samples read as 0.
 * spec[c*ld_spec + t*spec_stride + k] = {magnitude, phase}, k < spec_bins. */
pv_status pv_analysis(pv_handle* h, const float* x, long long ldx, long long n_samples,
                      int channels, int frames, pv_float2* spec, long long ld_spec, void* stream);

/* Processing + resynthesis of `frames` analysed frames per channel (spec is read only).
 * out[c*ldo + i], i < pv_output_length(h, frames): the full overlap-add.  ola_in
 * (nullable) holds N - out_hop samples per channel (stride ld_ola) already accumulated
 * at the start of this block (the reference's backFrame tail). */
pv_status pv_resynthesis(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                         int frames, const float* ola_in, long long ld_ola, float* out,
                         long long ldo, void* stream);

/* One long stream as consecutive non-empty frame segments s = 0, 1, ... (frames [f_s,
 * f_s + n_s) of every channel, e.g. one segment per GPU): segment s is analysed alone
 * (pv_analysis of x + f_s * hop), summarised (pv_segment_summary: per bin, its unwrap
 * decisions after its first frame and its first and last phase — pv_segment_summary_words(h)
 * int32 per channel, device memory [channels][words]), and after the summaries of segments
 * 0 .. s - 1 are known (gathered, in order, as [s][channels][words]), resynthesised by
 * pv_segment_resynthesis with frame0 = f_s: the unwrap counts and output phases are then those
 * of the whole stream bit for bit (integer sums; the boundary decisions are made on the GPU
 * with the contract's operations).  out holds the segment's own overlap-add,
 * pv_output_length(h, n_s) samples per channel starting at stream position f_s * out_hop;
 * its first N - out_hop samples overlap the previous segment's last ones (the caller adds
 * them).  STANDARD handles (REF_COMPAT has no unwrap state: pv_segment_resynthesis is then
 * pv_resynthesis).  pv_segment_summary of an empty segment is PV_ERR_ARG. */
int pv_segment_summary_words(const pv_handle* h);
pv_status pv_segment_summary(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                             int frames, int* summary, void* stream);
pv_status pv_segment_resynthesis(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                                 int frames, long long frame0, const int* summaries, int seg, float* out,
                                 long long ldo, void* stream);

/* analysis + processing + resynthesis (spec is the caller-owned spectrum buffer).  spec may
 * be NULL when the caller does not want the spectrum: on the single launch (pv_info.
 * single_launch = 1) it is then computed and consumed on chip and not written (SURVEY §8(d)
 * fused mode); on the split path it goes through the handle's own buffer (max_channels x
 * max_frames rows, zeroed, allocated by pv_reserve_spectrum or by the first such call:
 * PV_ERR_NOMEM if that fails; a first call made while `stream` is being captured returns
 * PV_ERR_ARG, since an allocation cannot be captured).  Either way, for pitch > 1 the bins
 * no output bin reads (above about L / scale) may be left unanalysed and are not read; the
 * output is the same bits as with a spectrum buffer. */
/* allocate (once, zeroed) the handle's own spectrum rows that pv_process(spec = NULL) uses
 * on the split path, so that such calls can then be captured into a graph; thread-safe; a
 * no-op for a single-launch handle (unless phase locking, formant preservation or
 * pv_pitch_set_formant is on).  Not
 * capturable itself (it allocates). */
pv_status pv_reserve_spectrum(pv_handle* h);

/* The channel-resident launch: pv_process(spec = NULL) with at least this many channels, on a
 * handle with phase locking, formant preservation, the envelope warp and the transient reset
 * off and x / out rows that are 8-byte aligned with even strides, runs one workgroup per
 * channel that keeps the spectrum rows on chip — the split path's output bits, no spectrum rows
 * (nothing is allocated, so such a call can be captured without pv_reserve_spectrum).  With
 * PV_RESIDENT unset the choice also ends at 1024 channels, one round of the kernel on the chip
 * (more take the split path); PV_RESIDENT=1 has no upper end.  0: this handle never takes it
 * (geometry or PV_RESIDENT=0); pv_info.single_launch stays 0 either way. */
int pv_resident_min_channels(const pv_handle* h);

pv_status pv_process(pv_handle* h, const float* x, long long ldx, long long n_samples,
                     int channels, int frames, pv_float2* spec, long long ld_spec, float* out,
                     long long ldo, void* stream);

/* Identity phase locking of the STANDARD time stretch (Laroche & Dolson).
 * 0 (default): every bin's output phase is propagated on its own.  1: in every frame a bin is
 * a peak if its magnitude is strictly above those of its neighbours at distance 1 and 2 that
 * lie in [0, N/2]; every bin takes the output-minus-analysis phase of the nearest peak (the
 * lower one on a tie; its own if the frame has no peak) and keeps its analysis phase relation
 * to that peak, so the bins of one partial stay coherent.  The analysis, the spectrum rows and
 * the unwrap decisions are unchanged.  With locking on, pv_resynthesis, pv_process and
 * pv_segment_resynthesis run the locked synthesis kernel; a single-launch handle takes the
 * split path (pv_info.single_launch reads 0, and pv_process(spec = NULL) then uses the
 * handle's own rows: pv_reserve_spectrum), and goes back to the single launch when locking
 * is turned off.
 * STANDARD + PV_TIME_SHIFT handles; otherwise PV_ERR_UNSUPPORTED.  Other values: PV_ERR_ARG.
 * A setup call (not capturable), ordered like the handle's compute calls: it takes effect
 * for the calls enqueued after it.  pv_rt has its own switch (pv_rt_set_phase_lock); the
 * harmoniser has none. */
pv_status pv_set_phase_lock(pv_handle* h, int lock);
int pv_get_phase_lock(const pv_handle* h);

/* Formant-preserving STANDARD pitch shift (cepstral spectral envelope).  The
 * plain pitch shift moves the spectral envelope with the partials (a voice shifted by 1.5 has
 * its formants 1.5 times too high).  With order > 0, per frame: lg[k] = ln max(mag[k], 2^-30)
 * (maxNum: a NaN magnitude gives the floor), k = 0 .. N/2, extended evenly to N points;
 * c = irfft(lg), c[n] = 0 wherever min(n, N - n) > order; le = Re rfft(c) is the log envelope;
 * output bin k' gets the magnitude exp(le[k']) * sum over its source bins k of
 * mag[k] * exp(-le[k]) (source order, zero without a source) and the plain pitch shift's phase:
 * the source is whitened, the excitation shifted, and the input's own envelope put back at the
 * target bin.  At ratio 1 the output is the plain one up to rounding.  The analysis, the spectrum
 * rows, the unwrap decisions and the stream segments are unchanged: the feature keeps no state
 * between frames.
 * order = 0 (default): off.  order in [1, N/4]: on.  Other values: PV_ERR_ARG.  STANDARD +
 * PV_PITCH_SHIFT handles; otherwise PV_ERR_UNSUPPORTED.  A setup call (not capturable), ordered
 * like the handle's compute calls.  The first call with order > 0 allocates, zeroed, the handle's
 * envelope rows: max_channels x max_frames rows of N/2 + 16 floats (bin N/2 and 15 zeros, so
 * that every row store is whole 64-byte segments), 4 (N/2 + 16) bytes per frame — about 3.6 GB
 * for 1024 channels x 861 frames at N = 2048; PV_ERR_NOMEM if that fails, and the feature stays
 * off.  While it is on, pv_resynthesis, pv_process and pv_segment_resynthesis run the envelope
 * kernel and then the formant synthesis kernel; a single-launch handle takes the split path
 * (pv_info.single_launch reads 0, pv_process(spec = NULL) uses the handle's own rows:
 * pv_reserve_spectrum) and goes back to the single launch with order 0; pv_process(spec = NULL)
 * analyses every bin (the envelope at the target bins reads magnitudes above N/2 / scale).
 * pv_rt has no such switch. */
pv_status pv_set_formant(pv_handle* h, int order);
int pv_get_formant(const pv_handle* h);

/* The log envelope rows of analysed frames, by the same kernel:
 * env[c*ld_env + t*(N/2 + 8) + k] = le[k], k = 0 .. N/2 (rows of N/2 + 8 floats — the natural
 * layout's spec_stride; a packed handle's N/2 slots cannot hold the N/2 + 1 values), order in
 * [1, N/4].  Any STANDARD handle, natural or packed spectrum rows; no state, capturable. */
pv_status pv_spectral_envelope(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels,
                               int frames, int order, float* env, long long ld_env, void* stream);

/* ---------------------------------------------------------------- resampler
 * Band-limited resampling by a rational ratio, and the pitch shift built on it.
 * p/q is reduced by its gcd to P/Q.  Output sample m sits at input position m P / Q: integer
 * part i_m = floor(m P / Q), phase r_m = (m P) mod Q (exact 64-bit integers); n_out =
 * ceil(n_in Q / P), every m with m P / Q < n_in.  P/Q > 1 reads faster: the pitch goes up and
 * the signal gets shorter.
 *   quality   0 fast: Z = 16, rolloff = 0.85,               Kaiser beta = 8.555504641634386
 *             1 best: Z = 64, rolloff = 0.9475937167399596, Kaiser beta = 14.769656459379492
 *   filter    s = rolloff min(1, Q/P), W = ceil(Z / s),
 *             h(tau) = s sinc(s tau) I0(beta sqrt(1 - u^2)) / I0(beta), u = s tau / Z, for
 *             |u| < 1 and 0 otherwise; sinc(x) = sin(pi x) / (pi x)
 *   output    y[m] = sum_{j = -W+1}^{W} x[i_m + j] h(j - r_m / Q); x reads as 0 outside
 *             [0, n_in), as pv_analysis reads it past n_samples
 * Ratio 1 (P = Q) is an exact copy with no filter.  Accepted: 1/4 <= P/Q <= 4 with P, Q <= 4096;
 * anything else is PV_ERR_UNSUPPORTED; quality other than 0, 1 and p or q <= 0 are PV_ERR_ARG.
 * The Q x 2W coefficients are built on the host in fp64 (I0 by its power series) and rounded
 * to fp32 once, by pv_resampler_create (it allocates: not capturable); the kernel accumulates in
 * fp32 in its own tap order, so the result is tolerance bound like the synthesis (no bit-exact
 * contract; pv_contract_version is not concerned). */
typedef struct pv_resampler pv_resampler;
pv_status pv_resampler_create(int p, int q, int quality, int device, pv_resampler** out);
void pv_resampler_destroy(pv_resampler* rs);
/* n_out for n_in input samples (0 for a NULL resampler or n_in <= 0) */
long long pv_resample_length(const pv_resampler* rs, long long n_in);
/* y[c*ldy + m], m < pv_resample_length(rs, n_in), from x[c*ldx + i], i < n_in, c < channels:
 * device pointers on the resampler's device; x and y must not overlap (PV_ERR_ARG).  channels
 * or n_in 0: nothing is done (PV_OK).  One launch, no allocation, no synchronisation: capturable. */
pv_status pv_resample(pv_resampler* rs, const float* x, long long ldx, long long n_in, int channels,
                      float* y, long long ldy, void* stream);

/* Pitch shift by time stretch and resampling, on a STANDARD + PV_TIME_SHIFT handle: the handle's
 * stretch by out_hop / hop, then a resampling by P/Q = out_hop / hop, restores the duration and
 * moves the pitch by the realised ratio out_hop / hop.  Unlike the bin-mapping PV_PITCH_SHIFT it
 * keeps the bins of a partial together, and it honours pv_set_phase_lock.
 * pv_pitch_reserve (a setup call, not capturable) builds the handle's resampler of the given
 * quality and allocates its scratch rows, max_channels x pv_output_length(h, max_frames) floats
 * (PV_ERR_NOMEM: the feature stays off); calling it again replaces the quality.
 * pv_pitch_process is exactly pv_process into the scratch rows, then pv_resample into out (same
 * arguments and spec semantics as pv_process, spec = NULL included; capturable under pv_process's
 * conditions); out[c*ldo + m], m < pv_pitch_output_length(h, frames) =
 * pv_resample_length of pv_output_length(h, frames).  At out_hop = hop it is pv_process, bit for
 * bit.
 * REF_COMPAT or PV_PITCH_SHIFT handle: PV_ERR_UNSUPPORTED; out_hop / hop outside [1/4, 4]:
 * PV_ERR_UNSUPPORTED; bad quality: PV_ERR_ARG; pv_pitch_process before a successful
 * pv_pitch_reserve: PV_ERR_ARG; NULL handle: PV_ERR_ARG (0 from the length call).
 * pv_rt has a streaming form (pv_rt_pitch_push); the harmoniser and the stream segments have
 * none. */
pv_status pv_pitch_reserve(pv_handle* h, int quality);
long long pv_pitch_output_length(const pv_handle* h, int frames);
pv_status pv_pitch_process(pv_handle* h, const float* x, long long ldx, long long n_samples,
                           int channels, int frames, pv_float2* spec, long long ld_spec, float* out,
                           long long ldo, void* stream);

/* Formant preservation for the pitch shift by time stretch and resampling.
 * The stretch keeps the spectral envelope in place and the resampling by out_hop / hop then
 * moves it with the partials.  With order > 0 every frame of the stretch is pre-warped so that
 * the resampling puts the envelope back where the input had it.  Per frame, with L = N/2 and
 * le[k] the log envelope of pv_set_formant (same order, same floor, same kernel):
 *   a = k out_hop, i_k = a div hop, r_k = a mod hop (exact integers); from the first bin with
 *   i_k >= L on, i_k = L and r_k = 0 (those bins land above the output's Nyquist frequency and
 *   the resampler's low-pass removes them);
 *   lw[k] = le[i_k] + (r_k / hop) (le[min(i_k + 1, L)] - le[i_k]);
 *   |Y[k]| = mag[k] exp(lw[k] - le[k]);
 * the output phase is the stretch's, unlocked or locked (pv_set_phase_lock: both settings
 * compose with this one); peaks and owners are decided on the frame's own magnitudes, the warp is
 * a positive real gain applied after every decision.  No state between frames: the analysis, the
 * spectrum rows, the unwrap decisions and the stream segments are unchanged.  At out_hop = hop the
 * gain is exp(0) = 1 and the output is the plain one.
 * order = 0 (default): off.  order in [1, N/4]: on.  Other values: PV_ERR_ARG.  STANDARD +
 * PV_TIME_SHIFT handles; REF_COMPAT or PV_PITCH_SHIFT: PV_ERR_UNSUPPORTED (pv_set_formant keeps
 * its meaning and its refusals).  NULL handle: PV_ERR_ARG (0 from the get call).  A setup call
 * (not capturable), ordered like the handle's compute calls.  The first call with order > 0
 * allocates, zeroed, the envelope rows of pv_set_formant (max_channels x max_frames rows of
 * N/2 + 16 floats; PV_ERR_NOMEM: the feature stays off) and uploads the warp map {i_k, r_k / hop}
 * (built on the host; not part of the exported tables: a tables_external handle builds its own).
 * While it is on, pv_resynthesis, pv_process and pv_segment_resynthesis run the envelope kernel
 * and then the warp synthesis kernel, so pv_pitch_process stays "pv_process into the scratch rows,
 * then pv_resample"; a single-launch handle takes the split path (pv_info.single_launch reads 0,
 * pv_process(spec = NULL) uses the handle's own rows: pv_reserve_spectrum) and goes back to the
 * single launch with order 0.
 * The feature is for harmonic-rich signals.  A lone sinusoid has no formants: its envelope is
 * the partial itself, and the warp attenuates it (DESIGN.md §3.10 has figures).
 * pv_rt and the harmoniser have no such switch. */
pv_status pv_pitch_set_formant(pv_handle* h, int order);
int pv_pitch_get_formant(const pv_handle* h);

/* Transient phase reset of the STANDARD time stretch.  The phase vocoder
 * advances every bin's output phase from the bin's own history; at a drum hit, a click or a
 * consonant that history says nothing about the new event, the bins of the attack frame no
 * longer line up, and the attack smears over a whole window.  With the feature on, a flagged
 * frame t0 is put down with its analysis phases (its waveform is the input's), and the frames
 * after it keep the offset that made it so: with closed(t)[k] the output phase of the plain
 * stretch,
 *   phi_s(t0)[k] = phi(t0)[k]
 *   phi_s(t)[k]  = closed(t)[k] + 2 pi Theta[k],  Theta[k] = frac((phi(t0)[k] - closed(t0)[k]) / 2 pi),
 * until the next flagged frame; Theta = 0 before the first one.  The unwrap decisions, the run
 * records and the carries are unchanged.  With pv_set_phase_lock on, a peak's output phase
 * includes its Theta and the locking is otherwise unchanged; at a flagged frame Y = X.  With no
 * frame flagged the output is the feature-off output of the split path bit for bit.
 *   PV_TRANSIENT_OFF     (default)
 *   PV_TRANSIENT_FLAGS   the frames flagged by pv_transient_set_flags
 *   PV_TRANSIENT_DETECT  the frames the detector flags in every pv_process call: with, per
 *       channel and frame, rise[t] = sum over bins 0 .. N/2 of max(0, mag_t[k] - mag_{t-1}[k])
 *       (mag_{-1} = 0) and tot[t] = sum of mag_t[k] (fp32 sums in the kernel's order; a NaN
 *       magnitude adds 0 to both), frame t >= 1 is flagged iff rise[t] > thr tot[t] and
 *       rise[t] > rise[t-1] and rise[t] >= rise[t+1] (rise[frames] = 0): the local maximum of
 *       the incoming energy inside a run of candidate frames.  The flags of the last call can be
 *       read with pv_transient_get_flags.
 * thr in (0, 1), or 0 for PV_TRANSIENT_DEFAULT_THRESHOLD.  Frame 0 is never flagged.
 * pv_set_transient is a setup call (not capturable), ordered like the handle's compute calls.
 * While the mode is not OFF, pv_process and pv_pitch_process run the reset synthesis (DETECT:
 * analysis, onset, pick, carry, reset, synthesis; profile names onset, pick, reset,
 * synthesis_reset); a single-launch handle takes the split path (pv_info.single_launch reads 0,
 * pv_process(spec = NULL) uses the handle's own rows: pv_reserve_spectrum).
 * pv_transient_reserve allocates, once and zeroed, the handle's flags (max_channels x max_frames
 * bytes), the {rise, tot} rows (8 bytes per frame), the reset offsets (max_channels x runs x
 * (N/2 + 1 padded) floats) and a word per run; PV_ERR_NOMEM if that fails.  It is not
 * capturable; the first pv_process / pv_transient_set_flags call without it allocates them, and
 * under a stream capture returns PV_ERR_ARG instead.
 * pv_transient_set_flags / _get_flags: device pointers, flags[c*ld + t] (a byte, != 0: flagged),
 * c < channels, t < frames, copied on `stream` (asynchronous, capturable once reserved); set
 * clears the rest of those channels' rows and frame 0's flag.
 * pv_onset_strength: dst[c*ld_dst + t] = {rise[t], tot[t]} of analysed frames, by the
 * detector's kernel; any STANDARD handle, natural or packed rows; no state, capturable.
 * Refusals, all PV_ERR_ARG with a pv_last_error text: a REF_COMPAT handle; a PV_PITCH_SHIFT
 * handle; pv_set_transient (mode not OFF) while pv_pitch_set_formant is on, and
 * pv_set_formant / pv_pitch_set_formant (order > 0) while the mode is not OFF; pv_segment_summary
 * and pv_segment_resynthesis while the mode is not OFF; pv_resynthesis while the mode is not
 * OFF; an unknown mode; thr outside (0, 1).  pv_rt and the harmoniser have no such switch. */
enum { PV_TRANSIENT_OFF = 0, PV_TRANSIENT_FLAGS = 1, PV_TRANSIENT_DETECT = 2 };
#define PV_TRANSIENT_DEFAULT_THRESHOLD 0.3f
pv_status pv_transient_reserve(pv_handle* h);
pv_status pv_set_transient(pv_handle* h, int mode, float thr);
int pv_get_transient(const pv_handle* h);
pv_status pv_transient_set_flags(pv_handle* h, const unsigned char* flags, long long ld, int channels,
                                 int frames, void* stream);
pv_status pv_transient_get_flags(pv_handle* h, unsigned char* flags, long long ld, int channels, int frames,
                                 void* stream);
pv_status pv_onset_strength(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels, int frames,
                            pv_float2* dst, long long ld_dst, void* stream);

/* Time-map stretch: an arbitrary, time-varying playback rate.  Output frame
 * u < n_out is built at the fractional analysis position pos[u] (in frames; one map for all
 * channels of a call unless set per channel, pv_timemap_set_channels below) with the synthesis hop equal to the analysis hop, so a tempo curve, a ratio
 * that is no multiple of 1/hop, a freeze (pos constant), a scrub and a reverse (pos decreasing)
 * are all maps.  The handle: STANDARD + PV_TIME_SHIFT with out_hop == hop (scale 1), natural or
 * packed rows, n_samps in [256, 2048]; the map replaces the scale.
 *   Map.  Every pos[u] finite, >= 0 and < 2^30; need not be monotonic; 1 <= n_out <= max_frames.
 *     Split once on the host (pv_timemap_split): i_u = (int)floor(pos[u]),
 *     a_u = (float)(pos[u] - floor(pos[u])).  At process time max_u i_u <= frames - 1.
 *   Phase as an integer.  For an analysed row's phase phi: t = phi * (1/2pi) (one fp32 multiply,
 *     the synthesis' constant 0x1.45f306p-3f), P = ((uint32_t)(int32_t)rintf(t * 0x1p31f)) << 1:
 *     a fraction of a turn in units of 2^-32 (the scaling is exact, nothing saturates, ties to even).
 *   Propagation, per channel and bin, modulo 2^32:
 *     Phi(0) = P(i_0),  Phi(u+1) = Phi(u) + Delta(i_u),
 *     Delta(i) = P(i+1) - P(i) for i + 1 < frames,  Delta(frames-1) = 0.
 *     The sum is exact and associative: the result does not depend on the run length.
 *   Magnitude.  m(u)[k] = fmaf(a_u, mag(i_u+1)[k] - mag(i_u)[k], mag(i_u)[k]) in fp32; row
 *     `frames`, one past the end, reads as magnitude 0 and is never loaded.
 *   Output phase.  Psi = Phi(u); with pv_set_phase_lock on, peaks and owners by the locking's
 *     rules on m(u), and Psi[k] = P(i_u)[k] + (Phi(u)[own] - P(i_u)[own]).
 *   Frame.  Y[k] = m(u)[k] (cos, sin)(2 pi Psi[k] / 2^32), Im Y(0) = Im Y(N/2) = 0; the inverse
 *     FFT, gain and overlap-add at `hop` are the handle's own.  Output length:
 *     pv_output_length(h, n_out).  With pos[u] = u, Psi = P(u), locked or not: pv_process at
 *     scale 1 up to the 2^-31-turn quantisation.
 * pv_timemap_split: pure host, no handle, no GPU; PV_ERR_ARG on NULL, n <= 0 or a position that
 *   is not finite, negative or >= 2^30.
 * pv_timemap_set: validates, splits and uploads the map; a setup call (not capturable), ordered
 *   like the handle's compute calls.  Its first call allocates, zeroed, the map (max_frames
 *   entries) and the scan's run sums and carries (max_channels x runs x (N/2 + 1 padded) uint32
 *   each); on PV_ERR_NOMEM the feature stays off.  n_out > max_frames: PV_ERR_ARG.
 *   pv_timemap_set(h, NULL, 0) clears the map.
 * pv_timemap_frames: n_out; 0 for a NULL handle or when no map is set.
 * pv_timemap_process: pv_process's arguments and `spec` semantics (frames: the analysed frames;
 *   spec = NULL uses the handle's own rows, pv_reserve_spectrum, never the single launch);
 *   out rows of pv_output_length(h, pv_timemap_frames(h)) samples.  Capturable under pv_process's
 *   conditions once a map is set.  Launches (and pv_profile_read names): analysis, map_sum,
 *   map_carry, synthesis_map, seam.  channels = 0 does nothing and returns PV_OK.
 * Refusals, each with a pv_last_error text: a NULL handle PV_ERR_ARG (0 from the count); a
 *   REF_COMPAT handle, a PV_PITCH_SHIFT handle, out_hop != hop: PV_ERR_UNSUPPORTED; process before
 *   a successful set, frames < 1 with channels > 0, max i_u > frames - 1, the transient mode not
 *   OFF, pv_pitch_set_formant on: PV_ERR_ARG.
 * A map per channel.  pv_timemap_set_channels: pos[c*ld_pos + u] is channel c's
 *   position for output frame u, u < counts[c] (counts in [1, n_out]; NULL: n_out for every
 *   channel; the entries from counts[c] on are not read).  Everything above holds per channel with
 *   its own map: Phi(0) = P(i_0) of the channel's own i_0, the same integer scan, the same
 *   magnitudes, pv_set_phase_lock composes.  Output frames u >= counts[c] of channel c contribute
 *   nothing: its row is pv_output_length(h, n_out) samples like every other, and its samples from
 *   pv_output_length(h, counts[c]) on are 0; below that it is, bit for bit, the row of
 *   pv_timemap_set(pos + c*ld_pos, counts[c]) and a call of that channel alone.  1 <= channels <=
 *   max_channels, 1 <= n_out <= max_frames, ld_pos >= n_out with more than one channel;
 *   pv_timemap_frames then reads n_out and pv_timemap_channels `channels`.  pv_timemap_process
 *   takes channels <= pv_timemap_channels(h), channel c with map c; "max i_u <= frames - 1" is
 *   checked over the call's channels and their counted frames.  A setup call, ordered like
 *   pv_timemap_set; the first one grows the map to max_channels x max_frames entries of 8 bytes
 *   (PV_ERR_NOMEM: the previous state stays).  pv_timemap_set (a shared map, or the clear) replaces
 *   a map per channel and the other way round; either turns a pitch map off.
 *   pv_timemap_channels: 0 for NULL, without a map, or with the shared one.
 *   PV_ERR_ARG, with the channel named in pv_last_error where one is at fault: NULL positions,
 *   channels, n_out or a count out of range, ld_pos < n_out, a position pv_timemap_split refuses
 *   among a channel's counted ones; at process time more channels than the map has.
 * pv_process and every other entry point are unchanged by a map. */
pv_status pv_timemap_split(const double* pos, int n, int* idx, float* frac);
pv_status pv_timemap_set(pv_handle* h, const double* pos, int n_out);
pv_status pv_timemap_set_channels(pv_handle* h, const double* pos, long long ld_pos,
                                  const int* counts /* nullable */, int channels, int n_out);
int pv_timemap_frames(const pv_handle* h);
int pv_timemap_channels(const pv_handle* h);   /* 0: no map, or the shared one */
pv_status pv_timemap_process(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels,
                             int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                             void* stream);

/* ---------------------------------------------------------------- variable-rate resampler
 * Band-limited resampling by a ratio that changes along the signal, and the pitch map built on
 * it.  The output is cut into blocks of B samples (`block`, fixed at creation,
 * 16 <= B <= 4096).  The map is a start position and one step per block, 64-bit integers in
 * units of 2^-32 input samples:
 *   positions T_0 = start >= 0, T_{b+1} = T_b + B d_b, all <= 2^62.  Output m = b B + j (j < B)
 *             reads the input at t_m = T_b + j d_b: i_m = t_m >> 32, fq_m = t_m & 0xffffffff,
 *             exact integers.  2^30 <= d_b <= 2^34 (ratio 1/4 .. 4): constant within a block,
 *             free to jump between blocks.  pv_varresample_steps: d = llrint(ratio 2^32).
 *   filter    per block, with pv_resampler_create's presets {Z, rolloff, beta}: Sq_b = the
 *             largest even 32-bit integer <= rolloff min(1, 2^32 / d_b) 2^32 (fp64),
 *             s_b = Sq_b / 2^32, W_b = ceil(Z / s_b), and h_b the resampler's h with s = s_b.
 *   output    y[m] = sum_{j = -W_b+1}^{W_b} x[i_m + j] h_b(j - fq_m / 2^32); x reads as 0
 *             outside [0, n_in) (masked: what lies there, a NaN included, is never loaded)
 * Every step 2^32 and a start without a fraction: the rows shifted by start >> 32, no filter.
 * No coefficient table can exist; the kernel computes every tap's coefficient in fp32 (the sine
 * from an exact integer fraction of a turn) and accumulates in fp32 in its own order: tolerance
 * bound like pv_resample, no bit-exact contract.
 * pv_varresampler_create allocates the device records of max_blocks blocks, zeroed (max_blocks
 *   * block < 2^31); pv_varresampler_set_map validates the map, builds the per-block records and
 *   the per-tile input spans on the host and uploads them between two synchronisations: setup
 *   calls, not capturable.  pv_varresample_length: nblocks * block, 0 without a map or for NULL.
 * pv_varresample: y[c*ldy + m], m < n_out <= pv_varresample_length, from x[c*ldx + i], i < n_in;
 *   device pointers on the resampler's device.  One launch (in a handle's profile:
 *   var_resample), no allocation, no synchronisation: capturable.  channels or n_out 0: nothing
 *   is done (PV_OK).
 * PV_ERR_ARG, each with a pv_last_error text: a NULL object or argument; quality other than 0, 1,
 *   block outside [16, 4096], max_blocks < 1; nblocks outside [1, max_blocks]; a step out of
 *   range; a negative start or positions past 2^62; pv_varresample before a map; n_out > length;
 *   x and y overlapping; ldx < n_in or ldy < n_out with more than one channel; a ratio that is
 *   not finite or outside [1/4, 4], or n <= 0.
 * Maps per channel.  pv_varresampler_set_maps: channel c starts at start[c] and
 *   has the steps step[c*ld_step + b], b < nblocks (the same nblocks for every channel); the
 *   validation, the records and the tile spans are pv_varresampler_set_map's per channel, and
 *   channel c of pv_varresample is, bit for bit, what that shared map gives the channel alone.  A
 *   channel whose steps are all 2^32 and whose start has no fraction is the shifted copy, whatever
 *   the other channels are.  A setup call; it allocates or grows the channels' records (about 24
 *   bytes per block and 16 per tile and channel; PV_ERR_NOMEM: the previous state stays).
 *   pv_varresample then takes channels <= pv_varresample_map_channels(vr) (0 for NULL, without a
 *   map, or with the shared one).  pv_varresampler_set_map replaces the maps per channel with the
 *   shared one, and the other way round.  PV_ERR_ARG also on channels < 1, ld_step < nblocks with
 *   more than one channel, and a call with more channels than the maps; the channel at fault is
 *   named in pv_last_error. */
typedef struct pv_varresampler pv_varresampler;
pv_status pv_varresampler_create(int quality, int block, int max_blocks, int device, pv_varresampler** out);
void pv_varresampler_destroy(pv_varresampler* vr);
pv_status pv_varresample_steps(const double* ratio, int n, long long* step);
pv_status pv_varresampler_set_map(pv_varresampler* vr, long long start, const long long* step, int nblocks);
pv_status pv_varresampler_set_maps(pv_varresampler* vr, int channels, const long long* start /* [channels] */,
                                   const long long* step, long long ld_step, int nblocks);
int pv_varresample_map_channels(const pv_varresampler* vr);   /* 0: no map, or the shared one */
long long pv_varresample_length(const pv_varresampler* vr);
pv_status pv_varresample(pv_varresampler* vr, const float* x, long long ldx, long long n_in, int channels,
                         float* y, long long ldy, long long n_out, void* stream);

/* Pitch map: a time-varying pitch ratio beside a time-varying tempo, as "time map, then
 * variable-rate resampling" (pv_pitch_process is "stretch, then pv_resample").  On the handles
 * pv_timemap_set accepts.  Per final output frame u < n the caller gives pos[u], the analysis
 * position that frame sounds at (the tempo curve: pv_timemap_set's map when the pitch is left
 * alone), and ratio[u], the pitch ratio there.  The output keeps pv_output_length(h, n) samples.
 *   Plan (pv_pitchmap_plan: pure host, no handle, no GPU; integers and fp64).  With N = n_samps,
 *     L = n hop + N - hop: nb = ceil(L / hop) blocks of hop samples with d_b = llrint(ratio[b]
 *     2^32), the last ratio repeated over the blocks b >= n.  Sigma_0 = 0, Sigma_{b+1} = Sigma_b
 *     + hop d_b: the resampler reads the stretched signal at Sigma.  The stretch has n_s =
 *     max(1, ceil(Sigma_n / (hop 2^32))) frames; frame v, at t = v hop 2^32, lies in the block
 *     b <= n - 1 with Sigma_b <= t < Sigma_{b+1}, w = (t - Sigma_b) / (Sigma_{b+1} - Sigma_b) (one
 *     fp64 division of exact integers), pos_s[v] = pos[b] + w (pos[min(b+1, n-1)] - pos[b]).
 *     Writes pos_s[*n_s] (at most 4 n + 1) and step[*n_steps] (nb).  PV_ERR_ARG on NULL, n < 1,
 *     n hop >= 2^28, hop < 1 or > n_samps, a position pv_timemap_split refuses, a ratio
 *     pv_varresample_steps refuses, or a capacity too small.
 *   pv_pitchmap_set plans, installs pos_s as pv_timemap_set does (pv_timemap_frames then reads
 *     n_s; n or n_s > max_frames: PV_ERR_ARG), and creates or re-maps the handle's variable-rate
 *     resampler (blocks of hop samples, 16 <= hop <= 4096).  A setup call.  Its first call
 *     allocates the scratch rows, max_channels x pv_output_length(h, max_frames) floats (those
 *     of pv_pitch_reserve); on PV_ERR_NOMEM the feature stays off.
 *     pv_pitchmap_set(h, NULL, NULL, 0, 0) clears the pitch map and its stretch map; a later
 *     pv_timemap_set by the caller, or its clear, turns the pitch map off too.
 *   pv_pitchmap_output_length: pv_output_length(h, n); 0 without a pitch map or for NULL.
 *   pv_pitchmap_process is exactly pv_timemap_process into the scratch rows, then pv_varresample
 *     into out: pv_timemap_process's arguments, `spec` semantics, capture conditions and
 *     refusals, plus PV_ERR_ARG without a pitch map.  Launches: pv_timemap_process's, then
 *     var_resample.  pv_set_phase_lock composes.  With ratio = 1 throughout it is
 *     pv_timemap_process of pos, bit for bit.
 *   pv_pitchmap_set_channels: pos[c*ld_pos + u] and ratio[c*ld_ratio + u], u < n,
 *     per channel c < channels <= max_channels.  The plan runs per channel; the stretch maps go in
 *     as pv_timemap_set_channels installs them, with counts n_s[c] and n_out = max_c n_s[c] (a
 *     channel whose n_s exceeds max_frames: PV_ERR_ARG, the channel named), the steps as
 *     pv_varresampler_set_maps does.  pv_pitchmap_process then takes channels <=
 *     pv_timemap_channels(h); channel c is, bit for bit, pv_pitchmap_set(pos + c*ld_pos, ratio +
 *     c*ld_ratio, n) run on that channel alone (a shorter channel's stretched samples up to the
 *     longest's length are exact zeros, which is what the resampler reads past a row's end), and
 *     a channel at ratio 1 throughout is pv_timemap_process of its positions.  The clear, the
 *     output length and the refusals are pv_pitchmap_set's.
 * One map for all channels unless set per channel.  pv_rt has a streaming form with a ratio per
 * pushed frame (pv_rt_pitchmap_push); the harmoniser, the stream segments and the envelope warp
 * have no pitch map.  pv_process and every other entry point are unchanged by
 * one. */
pv_status pv_pitchmap_plan(int n_samps, int hop, const double* pos, const double* ratio, int n, double* pos_s,
                           int cap_s, int* n_s, long long* step, int cap_steps, int* n_steps);
pv_status pv_pitchmap_set(pv_handle* h, const double* pos, const double* ratio, int n, int quality);
pv_status pv_pitchmap_set_channels(pv_handle* h, const double* pos, long long ld_pos, const double* ratio,
                                   long long ld_ratio, int channels, int n, int quality);
long long pv_pitchmap_output_length(const pv_handle* h);
pv_status pv_pitchmap_process(pv_handle* h, const float* x, long long ldx, long long n_samples, int channels,
                              int frames, pv_float2* spec, long long ld_spec, float* out, long long ldo,
                              void* stream);

/* Pitch tracker and correction curve: the fundamental frequency of every
 * analysed frame, and from it the pitch ratios that pv_pitchmap_set takes — analysis, track,
 * correction curve, pv_pitchmap_process without the spectrum leaving the device.
 * pv_pitch_track: dst[c*ld_dst + t] = {f0, strength}, c < channels, t < frames, from the rows'
 *   magnitudes mag[k], k <= N/2; f0 in cycles per sample, {0, 0} for a frame without a pitch.
 *   Any STANDARD handle (its window is the periodic Hann), natural or packed rows, n_samps in
 *   [256, 2048]; spec, ld_spec as pv_onset_strength's.  Per frame, with integer lags
 *   2 <= tau_min <= tau_max <= N/2 - 1 and kappa in (0, 1] (0: PV_PITCH_TRACK_DEFAULT_KAPPA):
 *     mx = max mag[k] (a NaN magnitude counts as 0); mx 0 or not finite: {0, 0}.
 *     s = 2^-e, e = mx's exponent taken from its bits (as at most 126);
 *     P[k] = (mag[k] s)^2 (NaN: 0), evenly extended to N points; r = irfft(P, N), the circular
 *     autocorrelation of the windowed frame; r[0] not above 0: {0, 0}.
 *     rho[n] = r[n] / (r[0] g[n]), g[n] = 2/3 + cos(2 pi n / N) / 3: the window's own
 *     autocorrelation divided out (Boersma's correction in its circular form).
 *     A lag n in [tau_min, tau_max] is a candidate iff rho[n] > rho[n-1], rho[n] >= rho[n+1]
 *     and rho[n] > 0; none: {0, 0}.  tau = the smallest candidate with rho >= kappa top, top the
 *     largest candidate's rho (McLeod and Wyvill's key maximum).  With a, b, c = rho[tau-1],
 *     rho[tau], rho[tau+1]: d = (a - c) / (2 (a - 2 b + c)), f0 = 1 / (tau + d),
 *     strength = b - (a - c) d / 4.
 *   fp32 in the kernel's order: tolerance bound (DESIGN.md §3.14 has the measured figures), no
 *   bit-exact contract, except that scaling the input by a power of two changes no bit.  The
 *   circular wrap grows with the lag: tau_max <= N/4 is the recommended range.  No voicing
 *   decision is made: the strength is the caller's to threshold (white noise stays below 0.5).
 *   No state between frames, nothing allocated; one launch (profile name: pitch), asynchronous
 *   on `stream`, capturable from the first call.  Nothing beyond `frames` entries per row is
 *   written.  channels = 0 or frames = 0 does nothing and returns PV_OK.
 *   Refusals, each with a pv_last_error text: a NULL handle, spec or dst, lags outside the range
 *   above, kappa outside [0, 1] or NaN, ld_spec < frames * spec_stride, ld_dst < frames with more
 *   than one channel: PV_ERR_ARG; a REF_COMPAT handle: PV_ERR_UNSUPPORTED.
 * pv_pitch_correct_plan: pure host, no handle, no GPU, fp64.  track: `frames` {f0, strength} of
 *   one voice in host memory; ratio[u], u < n: the pitch ratio of output frame u, which sounds at
 *   the analysis position pos[u] (NULL: pos[u] = u) — pv_pitchmap_set's two arrays.  cfg: a4,
 *   the frequency of A4 in cycles per sample, > 0; scale_mask, bit i set = pitch class i is
 *   allowed (0 = C), non-zero and below 2^12; strength_min, the voicing threshold; retune in
 *   (0, 1], 1 snaps at once.  With t = clamp(floor(pos[u] + 0.5), 0, frames - 1), frame u is
 *   voiced iff track[t].x is finite and > 0 and track[t].y >= strength_min (a NaN is unvoiced);
 *   then note = 69 + 12 log2(f0 / a4), target = the nearest allowed semitone (the lower one on a
 *   tie), c[u] = (target - note) / 12 octaves; unvoiced, c[u] = s[u-1]: the correction is held.
 *   s[-1] = 0, s[u] = s[u-1] + retune (c[u] - s[u-1]), ratio[u] = 2^s[u] clamped to [1/4, 4].
 *   PV_ERR_ARG with a pv_last_error text: a NULL track, cfg or ratio, frames or n < 1,
 *   cfg->abi_version != PV_ABI_VERSION, a field of cfg outside its range, a position that is not
 *   finite.
 * One correction curve per call: one voice, or channels that share a voice; a batch of voices is
 * one call per channel's track and one pv_pitchmap_set_channels (pv_pitchmap_set is one map for
 * all channels unless set per channel).  pv_rt and pv_main have no tracker: a live correction
 * tracks the rows pv_rt_pitchmap_push returns with pv_pitch_track on a batch handle of the same
 * geometry and feeds the next callback's ratios. */
#define PV_PITCH_TRACK_DEFAULT_KAPPA 0.9f
typedef struct pv_pitch_correct {
    int abi_version;      /* = PV_ABI_VERSION */
    double a4;
    unsigned scale_mask;
    double strength_min;
    double retune;
} pv_pitch_correct;
pv_status pv_pitch_track(pv_handle* h, const pv_float2* spec, long long ld_spec, int channels, int frames,
                         int tau_min, int tau_max, float kappa, pv_float2* dst, long long ld_dst, void* stream);
pv_status pv_pitch_correct_plan(const pv_float2* track, int frames, const double* pos, int n,
                                const pv_pitch_correct* cfg, double* ratio);

/* ---------------------------------------------------------------- real-time mode
 * A pv_rt streams `channels` mono channels through the STANDARD pipeline one callback at a
 * time.  State (input history, previous phases, unwrap counts, overlap accumulator) lives
 * on the device between calls.  A push of `nframes` frames consumes nframes*hop new
 * samples per channel and emits nframes*out_hop final samples per channel; the emitted
 * stream equals pv_process() of the same stream prefixed with N - hop zeros.
 * Supported: PV_MODE_STANDARD, n_samps in [256, 2048]. */
typedef struct pv_rt pv_rt;

pv_status pv_rt_create(const pv_config* cfg, int channels, pv_rt** out);
void pv_rt_destroy(pv_rt* rt);
/* zero the stream state (start of a new stream) */
pv_status pv_rt_reset(pv_rt* rt, void* stream);
/* device pointers: in[c*ldi + i], i < nframes*hop; out[c*ldo + i], i < nframes*out_hop;
 * spec (nullable) receives the analysed {mag, phase} rows: spec[c*ld_spec + f*spec_stride + k] */
pv_status pv_rt_push(pv_rt* rt, const float* in, long long ldi, int nframes, float* out,
                     long long ldo, pv_float2* spec, long long ld_spec, void* stream);
/* Capture one callback of `nframes` frames into a hipGraph: pinned host input -> device,
 * pv_rt_push, device -> pinned host output.  The pinned buffers are planar
 * [channels][nframes*hop] and [channels][nframes*out_hop] (pv_rt_host_buffers); after
 * pv_rt_pitch_reserve or pv_rt_pitchmap_reserve (below) the callback is pv_rt_pitch_push or
 * pv_rt_pitchmap_push, whichever reserve succeeded later, and the output buffer
 * [channels][nframes*hop]. */
pv_status pv_rt_capture(pv_rt* rt, int nframes);
pv_status pv_rt_host_buffers(pv_rt* rt, float** host_in, float** host_out);
/* One synchronous callback on the captured graph: copies `in` (host, planar, may be the
 * pinned buffer itself) into the pinned input, replays the graph, waits, copies the
 * result to `out` (host, may be the pinned output itself). */
pv_status pv_rt_callback(pv_rt* rt, const float* in, float* out);

/* Identity phase locking of the real-time time stretch: pv_set_phase_lock's semantics (above)
 * on a pv_rt.  With locking on, pv_rt_push runs the locked form of its kernel and the emitted
 * stream equals the locked pv_process() of the stream prefixed with N - hop zeros, frame for
 * frame; the analysis, the spectrum rows and the unwrap decisions are unchanged and locking
 * adds no stream state.  STANDARD + PV_TIME_SHIFT only, else PV_ERR_UNSUPPORTED; values other
 * than 0, 1: PV_ERR_ARG.  A setup call: PV_ERR_ARG while a callback is captured (call it
 * before pv_rt_capture). */
pv_status pv_rt_set_phase_lock(pv_rt* rt, int lock);
int pv_rt_get_phase_lock(const pv_rt* rt);

/* Real-time pitch shift by time stretch and streaming resampling: a callback
 * takes nframes*hop samples and gives nframes*hop pitch-shifted samples (ratio out_hop / hop)
 * at a fixed latency.  It honours pv_rt_set_phase_lock.
 *   S[n], n >= 0, is the stretched stream pv_rt_push would emit; S[n] = 0 for n < 0.
 *   P/Q = out_hop / hop reduced; W, the filter h and the presets are pv_resampler_create's.
 *   For every integer m, negative included:
 *       y[m] = sum_{j = -W+1}^{W} S[i_m + j] h(j - r_m / Q),
 *       i_m = floor(m P / Q) (toward -inf), r_m = m P mod Q in [0, Q).
 *   The emitted stream is z[m'] = y[m' - D], m' >= 0, with D = floor(W Q / P) output samples
 *   of latency (pv_rt_pitch_latency): the smallest delay at which every callback's outputs
 *   read only stretched samples that callback or an earlier one has produced.
 * A push of nframes frames consumes nframes*hop samples and emits exactly nframes*hop
 * (out_hop Q / P = hop).  At out_hop = hop it is pv_rt_push bit for bit, with D = 0.  The stream
 * does not depend on how it is cut into pushes (bit for bit), and no sample counter is kept: it
 * can run for ever.  Accumulation is fp32 in the kernel's own tap order (tolerance bound, like
 * pv_resample).
 * pv_rt_pitch_reserve (a setup call: allocates, not capturable; PV_ERR_ARG while a callback is
 * captured) builds the [Q][2W] coefficient table (fp64 on the host, rounded to fp32 once) and
 * the per-channel scratch rows [H history | max_nframes*out_hop new stretched samples],
 * H = 2W rounded up to a multiple of 4, zeroed; calling it again replaces quality and capacity
 * and restarts the resampler's history.  pv_rt_reset zeroes the history too.
 * pv_rt_pitch_push is pv_rt_push into the scratch rows, then one more launch (profile name
 * rt_resample); same arguments as pv_rt_push, but out[c*ldo + i], i < nframes*hop.  No
 * allocation, no synchronisation: capturable.  After a successful reserve pv_rt_capture
 * captures pv_rt_pitch_push (nframes <= max_nframes, else PV_ERR_ARG) and the pinned output
 * buffer is [channels][nframes*hop].
 * PV_PITCH_SHIFT handle: PV_ERR_UNSUPPORTED; out_hop / hop outside [1/4, 4]:
 * PV_ERR_UNSUPPORTED; bad quality, max_nframes <= 0 (or so large that max_nframes*hop*P
 * leaves 31 bits): PV_ERR_ARG; pv_rt_pitch_push before a successful reserve or with
 * nframes > max_nframes: PV_ERR_ARG; allocation failure: PV_ERR_NOMEM, and the feature stays
 * off.  pv_rt_pitch_latency: 0 for a NULL rt or before a reserve. */
pv_status pv_rt_pitch_reserve(pv_rt* rt, int quality, int max_nframes);
int pv_rt_pitch_latency(const pv_rt* rt);
pv_status pv_rt_pitch_push(pv_rt* rt, const float* in, long long ldi, int nframes, float* out,
                           long long ldo, pv_float2* spec, long long ld_spec, void* stream);

/* Real-time pitch map: pv_pitchmap_process as a stream.  Every pushed frame
 * carries one fp32 pitch ratio per channel, read from device memory when the launch runs, so a
 * captured callback is steered by writing its ratio buffer.  It honours pv_rt_set_phase_lock.
 * The pv_rt must be STANDARD + PV_TIME_SHIFT with out_hop == hop.  Per channel:
 *   rows     row t >= 0 is analysis frame t of the stream prefixed with N - hop zeros (pv_rt_push's
 *            analysis, bit for bit); P(t) its phases as 32-bit fractions of a turn (pv_timemap_*).
 *   steps    pushed frame t carries r_t; r' = min(max(r_t, ratio_min), ratio_max), a NaN reading as
 *            ratio_min; d = (int64)(r' 2^32), exact.  Frame 0's ratio is read and ignored; for
 *            t >= 1, d_{t-1} = d.  Span b runs from row b to row b+1 with the step d_b, and is built
 *            by the callback that analyses row b+1.  Sigma_0 = 0, Sigma_{b+1} = Sigma_b + hop d_b
 *            (64-bit, units of 2^-32 samples).
 *   stretch  stretched frame v, at t_v = v hop 2^32, lies in the span b with Sigma_b <= t_v <
 *            Sigma_{b+1} (0 to 4 per span): pv_timemap_process's frame at position b + a,
 *            a = (float)((double)(t_v - Sigma_b) / (double)(hop d_b)): magnitude fmaf(a, mag(b+1) -
 *            mag(b), mag(b)); Phi(0) = P(0), Phi += P(b+1) - P(b) modulo 2^32 after every stretched
 *            frame of span b; Psi = Phi, or locked P(b)[k] + (Phi - P(b))[own(k)] with the peaks
 *            and owners of the interpolated magnitudes.  Gain and overlap-add at `hop` are the
 *            handle's.  S is the resulting stream, S[n] = 0 for n < 0.
 *   output   block b, hop samples: sample j reads S at T = Sigma_b + j d_b through
 *            pv_varresample's filter of a block with step d_b (Sq_b, W_b, h_b as there; computed on
 *            the device in fp64 by the same operations).  No copy shortcut at ratio 1.
 *   latency  with d_min, d_max the steps of ratio_min, ratio_max and W_max = W(d_max):
 *            G = ceil(W_max 2^32 / (hop d_min)).  Pushed frame t emits block t - 1 - G (zeros below
 *            block 0): emitted sample m' is y[m' - (G+1) hop], and pv_rt_pitchmap_latency is
 *            (G+1) hop.  G callbacks are what it takes for every stretched sample a block reads to
 *            be final.  [0.84, 1.19], fast preset, hop >= 64: G = 1; [1/4, 4]: G = 5 at hop 64.
 * A push of nframes frames consumes nframes*hop samples and emits exactly nframes*hop.  The stream
 * does not depend on how it is cut into pushes (bit for bit); no state grows with its length (the
 * positions are relative to the scratch row, the counters saturate).  Tolerance bound like
 * pv_pitchmap_process, no bit-exact contract for the samples.
 * pv_rt_pitchmap_reserve (a setup call: allocates, not capturable) sizes and zeroes the state for
 *   pushes of up to max_nframes frames; calling it again replaces preset, range and capacity and
 *   zeroes the pitch map's own state (not the input history and the overlap accumulator it
 *   shares with pv_rt_push: pv_rt_reset starts a new stream).  PV_ERR_UNSUPPORTED: a PV_PITCH_SHIFT handle, out_hop != hop,
 *   hop < 16.  PV_ERR_ARG: a captured callback exists, bad quality, max_nframes <= 0, a range
 *   outside [1/4, 4], with ratio_min > ratio_max or with a NaN, G > 64, (G + max_nframes) hop >=
 *   2^28.  PV_ERR_NOMEM: nothing changes (the feature stays off if it was).  The later successful
 *   call of this or pv_rt_pitch_reserve decides what pv_rt_capture records.
 * pv_rt_pitchmap_latency: 0 for NULL or before a successful reserve.
 * pv_rt_pitchmap_push: device pointers; in, out, spec as pv_rt_push's with out[c*ldo + i],
 *   i < nframes*hop; ratio[c*ldr + f], f < nframes, or NULL for 1 throughout.  Two launches
 *   (profile names rt_map, rt_varresample), no allocation, no synchronisation: capturable.
 *   PV_ERR_ARG before a successful reserve, with nframes > max_nframes, or ldr < nframes with more
 *   than one channel.
 * pv_rt_pitchmap_host_ratios: after pv_rt_capture recorded pv_rt_pitchmap_push, the pinned
 *   [channels][nframes] buffer the captured callback reads its ratios from (device-mapped like the
 *   input buffer; a copy node where the runtime cannot map it), filled with 1 by the capture.
 *   PV_ERR_ARG without such a capture.
 * pv_rt_reset zeroes the pitch map's state too.  Switching between pv_rt_push, pv_rt_pitch_push
 * and pv_rt_pitchmap_push in mid-stream without a reset gives a finite, in-bounds but unspecified
 * stream.  Every refusal sets a pv_last_error text. */
pv_status pv_rt_pitchmap_reserve(pv_rt* rt, int quality, int max_nframes, float ratio_min, float ratio_max);
int pv_rt_pitchmap_latency(const pv_rt* rt);
pv_status pv_rt_pitchmap_push(pv_rt* rt, const float* in, long long ldi, int nframes, const float* ratio,
                              long long ldr, float* out, long long ldo, pv_float2* spec, long long ld_spec,
                              void* stream);
pv_status pv_rt_pitchmap_host_ratios(pv_rt* rt, float** host_ratio);

/* Real-time harmoniser: V voices of the real-time pitch map per channel from one
 * analysis of each pushed frame, mixed with a gain per voice and frame.  Two launches per callback
 * whatever V is.  It honours pv_rt_set_phase_lock.  Per channel c and voice v:
 *   voice    y_v is pv_rt_pitchmap_push's stream of the channel's input with the voice's ratios:
 *            the same rows, clamp (a NaN ratio reads as ratio_min), steps, spans, stretched frames,
 *            block filter and tap order, frame 0's ratio ignored, the same latency (G+1) hop with G
 *            from the ratio range: common to all voices.  No voice depends on another.
 *   gain     the gain pushed with frame t >= 1 belongs to output block b = t - 1, the block the
 *            ratio pushed with frame t steers, and waits with the step through the latency.  Frame
 *            0's gain is ignored; a NaN gain reads as 0; nothing else is clamped.  Sample j of block
 *            b has g(j) = fmaf((float)(j+1) * (1.0f / (float)hop), g_b - g_prev, g_prev) with
 *            g_prev = g_{b-1}, g_{-1} = g_0: a linear ramp over the block (a voice that turns on or
 *            off does not click), exactly g_b when the gain does not change.
 *   mix      mix[j] = fmaf(g_{V-1}(j), y_{V-1}[j], ... fmaf(g_0(j), y_0[j], +0)), the voices in
 *            rising order, fp32.  Blocks below block 0 are zeros.
 * There is no dry path of its own: a voice at ratio 1 is the input behind the same latency (the
 * identity map), which is how a caller adds the dry signal aligned with the wet one.
 * pv_rt_harmonizer_max_voices: pure host; 8, 8, 8, 4 for n_samps 256, 512, 1024, 2048, else 0.
 * pv_rt_harmonizer_reserve (a setup call: allocates, not capturable): pv_rt_pitchmap_reserve's
 *   preconditions and refusals, and PV_ERR_ARG for voices outside [1, max_voices(n_samps)].
 *   Calling it again replaces voices, preset, range and capacity and zeroes the harmoniser's state.
 *   PV_ERR_NOMEM: nothing changes (the feature stays off if it was).  The later successful call of
 *   this, pv_rt_pitchmap_reserve or pv_rt_pitch_reserve decides what pv_rt_capture records.
 * pv_rt_harmonizer_voices, pv_rt_harmonizer_latency: 0 for NULL or before a successful reserve.
 * pv_rt_harmonizer_push: device pointers; in, spec as pv_rt_pitchmap_push's; ratio and gain
 *   [channels][voices][nframes], element (c*V + v)*ld_ctl + f (ratio NULL: 1 throughout, gain NULL:
 *   1 / V); mix[c*ldo + i], i < nframes*hop; voices_out (nullable) [voices][channels][nframes*hop],
 *   element (v*channels + c)*ld_voice + i: every voice's own stream.  Two launches (profile names
 *   rt_hmap, rt_hresample), no allocation, no synchronisation: capturable.  PV_ERR_ARG before a
 *   successful reserve, with nframes > max_nframes, or with ld_ctl < nframes.
 * pv_rt_harmonizer_host_controls: after pv_rt_capture recorded pv_rt_harmonizer_push (its callback
 *   emits the mix), the pinned [channels][voices][nframes] buffers the captured callback reads its
 *   ratios and gains from, filled with 1 and 1 / V by the capture (either argument may be NULL).
 *   PV_ERR_ARG without such a capture.
 * pv_rt_reset zeroes the harmoniser's state too; it shares the input history with the other pushes,
 * so switching between them in mid-stream without a reset gives a finite, in-bounds but unspecified
 * stream.  Every refusal sets a pv_last_error text. */
int pv_rt_harmonizer_max_voices(int n_samps);
pv_status pv_rt_harmonizer_reserve(pv_rt* rt, int voices, int quality, int max_nframes, float ratio_min,
                                   float ratio_max);
int pv_rt_harmonizer_voices(const pv_rt* rt);
int pv_rt_harmonizer_latency(const pv_rt* rt);
pv_status pv_rt_harmonizer_push(pv_rt* rt, const float* in, long long ldi, int nframes, const float* ratio,
                                const float* gain, long long ld_ctl, float* mix, long long ldo, float* voices_out,
                                long long ld_voice, pv_float2* spec, long long ld_spec, void* stream);
pv_status pv_rt_harmonizer_host_controls(pv_rt* rt, float** host_ratio, float** host_gain);

/* ---------------------------------------------------------------- harmoniser
 * K voices, voice k = PITCH_SHIFT by ratios[k] of the same input, all from ONE analysis
 * and one unwrap scan (cfg: STANDARD; effect and scale are ignored).  voices_out[k*ld_voice
 * + c*ldo + i], i < pv_output_length (every voice has out_hop = hop); each voice equals
 * pv_process() with its ratio.  mix (nullable): mix[c*ld_mix + i] = sum_k gains[k] * voice
 * k (gains: host array of K floats).  spec (required) receives the shared analysis, as
 * pv_process's.  At most 64 voices.  channels or frames 0: nothing is done (PV_OK). */
typedef struct pv_harmonizer pv_harmonizer;
pv_status pv_harmonizer_create(const pv_config* cfg, const float* ratios, int voices, pv_harmonizer** out);
void pv_harmonizer_destroy(pv_harmonizer* hz);
pv_status pv_harmonize(pv_harmonizer* hz, const float* x, long long ldx, long long n_samples,
                       int channels, int frames, pv_float2* spec, long long ld_spec, float* voices_out,
                       long long ldo, long long ld_voice, const float* gains, float* mix,
                       long long ld_mix, void* stream);
/* pv_set_formant for every voice (same arguments and refusals): the envelope is computed once
 * per pv_harmonize call from the shared analysis into voice 0's rows, which every voice reads */
pv_status pv_harmonizer_set_formant(pv_harmonizer* hz, int order);

/* ---------------------------------------------------------------- standalone FFT
 * Batched unnormalised complex FFT (both directions, like the reference's GPU_FFT):
 * out[b*n + k] = sum_j in[b*n + j] * exp(-+2 pi i jk/n), b < batch, n a power of two in
 * [2, 2048]; in == out (in place) is allowed.  inverse != 0 uses exp(+...).  Device
 * pointers on the current HIP device; the first call per (device, n) builds that size's
 * twiddle table (allocation: not capturable), later calls are. */
pv_status pv_fft_c2c(const pv_float2* in, pv_float2* out, int n, int batch, int inverse, void* stream);

/* REF_COMPAT: replace the handle's window by the caller's (device pointer, n_samps
 * floats; copied on `stream`, the pointer is not kept).  The reference passes the window
 * to every call (CudaPhase::pv_analysis_CUFFT / resynthesis_CUFFT `win`, kernel.cu:301
 * and :406): it multiplies the analysis frame and the resynthesised frame.  Here the
 * analysis window becomes `win` and the synthesis gain win[k]/N (cudaDivVec kernel.cu:380
 * then cudaWindow :406).  STANDARD handles: PV_ERR_UNSUPPORTED (their synthesis
 * normalisation is derived from the Hann window at pv_create). */
pv_status pv_set_window(pv_handle* h, const float* win, void* stream);

/* Constant tables of a handle (windows, gains, twiddles, unwrap tables, pitch map) as one
 * device blob, so that one rank can build them and the others receive them over RCCL
 * (DESIGN.md §6).  export with dst == NULL only reports *bytes.  import validates the
 * blob's header against the handle's configuration and replaces the tables. */
pv_status pv_export_tables(const pv_handle* h, void* dst, size_t cap, size_t* bytes, void* stream);
pv_status pv_import_tables(pv_handle* h, const void* src, size_t bytes, void* stream);

/* kernel.cu:289-298 (OVERLAPTEST, main.cpp:156-202): identity processing of one frame,
 * out[k] = win[k]^2 * in[k] + (k + hop < N ? back[k + hop] : 0).  Device pointers. */
pv_status pv_test_overlap_add(const float* in, const float* win, const float* back, float* out,
                              int n, int hop, void* stream);

/* Per-kernel timing with hipEvents recorded on the launch stream (for bench.py).  enable:
 * 0 off, 1 every launch, k > 1 the launches of every k-th pv_analysis / pv_resynthesis /
 * pv_process / pv_rt_push call (an event record costs the queue a few us).  Within one call
 * the launches share events: launch i+1's timing starts at launch i's stop event, so any
 * GPU idle time while the host enqueues launch i+1 counts toward launch i+1 (a bias of a few
 * us at most, visible only on the short carry / seam launches). */
pv_status pv_profile_enable(pv_handle* h, int enable);
/* names[i] (static strings), total ms and launch count of each kernel since the last
 * reset; returns number of kernels written (<= cap). Synchronises the recorded events. */
int pv_profile_read(pv_handle* h, const char** names, double* total_ms, int* launches, int cap);
void pv_profile_reset(pv_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* PV_H */
