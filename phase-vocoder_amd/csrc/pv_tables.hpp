// pv_tables.hpp — the arithmetic behind a handle: table recipes, the rational output-phase
// factor, the pitch map, the run-length choices and the resampler's coefficients.
// Plain C++17 on the host, no HIP header and no device call: every value the numerics contract
// rests on can be computed, compared with the oracle and sanitised without a GPU
// (host/tables_dump.cpp, tests/test_tables_host.py).  Each formula is the oracle's (pvref.c) in
// its exact form and evaluation order; built with -ffp-contract=off like the rest.
#pragma once
#include <vector>

#include "../../include/pv.h"

#pragma GCC visibility push(hidden)
namespace pvtab {

constexpr double kPi = 3.14159265358979323846;
// rounds of workgroups are counted on the MI355X's CUs whatever device a handle is on
constexpr int kRoundCUs = 256;

bool is_pow2(long long v);

// ---- windows, synthesis gains (STANDARD; REF_COMPAT: win / N), twiddles
void hann_periodic(int N, std::vector<float>& w);
void hann_ref(int N, std::vector<float>& w);
void hamming_ref(int N, std::vector<float>& w);
void std_gain(int N, int hs, std::vector<float>& gain);
void compat_gain(const std::vector<float>& win, std::vector<float>& gain);
pv_float2 tw_entry(long long m, long long L);
void stage_twiddles(int L, std::vector<pv_float2>& t);
void fft_table(int L, std::vector<pv_float2>& t, bool v3 = false);
int tw_syn_len(int L);
void tw_syn_table(int L, std::vector<pv_float2>& t);  // the whole d_tw_syn block, tw_syn_len(L) entries
void split_twiddles(int N, std::vector<pv_float2>& t);

// ---- geometry of a configuration (phaseVocoder.h:79, :104)
struct Geometry {
    int hop, hs, pitch, L_ana, L_syn, bins, bins_pad, tail_len;
};
Geometry geometry(int N, int hop_div, int mode, int effect, float scale);

// ---- unwrap tables and the rational output-phase factor rho = p/q
struct PhaseTables {
    std::vector<float> ek;
    std::vector<long long> jk;
    std::vector<unsigned> jk_mod;  // (p_mod * (j_k mod q)) mod q
    float rho = 1.0f, inv_q = 1.0f;
    unsigned long long p = 1, q = 1, p_mod = 0;
    int q_pow2 = 1;
};
void phase_tables(int N, const Geometry& g, float scale, PhaseTables& t);
// every bin k < L repeats bin k mod 64, and bin L's e equals bin 0's (feeds k_lane)
bool bins_repeat_mod64(const PhaseTables& t);

// ---- pitch map: k' = floor(beta*k + 0.5) (magnitudes summed, phase from smallest k)
struct PitchMap {
    std::vector<int> first, cnt;
    int src_hi = 0;  // highest analysis bin any output bin reads (bins - 1 without a map)
};
void pitch_map(int bins, bool pitch, float scale, PitchMap& m);

// ---- envelope warp of the stretch-and-resample pitch shift (pv_pitch_set_formant; DESIGN.md
// §3.10): bin k reads the frame's log envelope at k out_hop / hop = idx[k] + frac[k], clamped
// to {L, 0}.  Not part of the exported table blob.
void warp_map(int bins, int hop, int out_hop, std::vector<int>& idx, std::vector<float>& frac);

// ---- time map (pv_timemap_split): pos[u] -> {floor, fp32 fraction}; false (idx / frac then
// partly written) on a position that is not finite, negative or >= 2^30
bool timemap_split(const double* pos, int n, int* idx, float* frac);

// ---- environment overrides (pv.h lists them), read once per pv_create
struct EnvOverrides {
    int compat_ana_frames = 4;                 // PV_COMPAT_ANA_FRAMES in [1, 256]
    int fused_half = 1, fused_balance = 1;     // PV_FUSED_HALF=0, PV_FUSED_BALANCE=0
    int run_frames = 0, fused_frames = 0;      // PV_RUN_FRAMES, PV_FUSED_FRAMES as given (0: unset)
    int fused = 1, syn_lanek = 1;              // PV_FUSED=0, PV_SYN_LANEK=0
    int resident = -1;                         // PV_RESIDENT: 0 never, 1 whenever supported, -1 unset
};
EnvOverrides read_env_overrides();

// ---- run lengths
// choose_run_frames fits F to whole rounds: the caller then asks the analysis kernel for its
// workgroups per CU and waves per workgroup (pv::std_analysis_wgs_per_cu)
bool run_fit_applies(long long work, int L_syn, int L_ana, int mode);
// frames per wave-run F; wgs_per_cu <= 0: no round fit.  C, T: max_channels, max_frames (>= 1)
int choose_run_frames(long long work, int L_syn, int L_ana, int mode, int wgs_per_cu, int waves_per_wg,
                      long long C, long long T, int hs, int tail_len, const EnvOverrides& env);
// frames per run of the single launch (q = 1), 0 with PV_FUSED=0
int choose_fused_frames(int F, long long work, int hs, int tail_len, const EnvOverrides& env);
// workgroups of the single launch and, when its rounds are balanced, the runs one frame longer
void fused_rounds(int frames, int F, bool balance, int* nwg, int* n4);
// The channel-resident kernel (pv_resident.hip) serves this handle geometry: a STANDARD time
// stretch (no pitch map) at N = 1024, hop N/4, out hop 128, whose output-phase denominator q is
// a power of two in [2, 4096] with per-lane unwrap constants, and whose runs cover the overlap.
struct ResidentGeometry {
    int mode, pitch, L_ana, L_syn, hop, hs, q_pow2, k_lane, F, tail_len;
    unsigned long long q;
};
bool resident_supported(const ResidentGeometry& g);
// the fewest channels from which pv_process(spec = NULL) takes the resident kernel on a
// supported handle; 0: never.  Unset, PV_RESIDENT leaves the measured threshold
// kResidentAutoChannels (profiles/resident_c3.txt).
constexpr int kResidentAutoChannels = 1024;
// one round of the kernel on the MI355X: 4 workgroups on each of 256 CUs.  Unset, PV_RESIDENT
// takes the kernel for channel counts from the threshold up to this.
constexpr int kResidentRoundChannels = 1024;
int resident_min_channels(bool supported, const EnvOverrides& env);

// ---- resampler presets (include/pv.h)
double bessel_i0(double x);
long long gcd_ll(long long a, long long b);
int resample_half_width(int P, int Q, int quality);
void resample_row(int P, int Q, int quality, int W, int r, float* row);
long long resample_length(int P, int Q, long long n_in);

// ---- variable-rate resampler and pitch map (include/pv.h)
constexpr long long kVarOne = 1LL << 32, kVarStepMin = 1LL << 30, kVarStepMax = 1LL << 34;
// d = llrint(ratio 2^32); false on a ratio that is not finite or outside [1/4, 4]
bool varresample_steps(const double* ratio, int n, long long* step);
// a block's cutoff Sq (even, s = Sq / 2^32) and half width W for its step d
void var_block_filter(long long d, int quality, unsigned* Sq, int* W);
double resample_zero_crossings(int quality);  // Z of the preset
double resample_rolloff(int quality);         // its rolloff
// the kernel's window table: n intervals over |u| in [0, 1], `len` > n entries {value / pi, rise}
void var_window_table(int quality, int n, int len, std::vector<float>& tab);
// pos, ratio [n] -> pos_s [n_s], step [ceil((n hop + N - hop) / hop)]; false on a bad argument
bool pitchmap_plan(int N, int hop, const double* pos, const double* ratio, int n, std::vector<double>& pos_s,
                   std::vector<long long>& step);

// ---- real-time pitch map (pv_rt_pitchmap_reserve): what follows from the hop,
// the preset, the ratio range and the largest push.  d_min, d_max: the steps (int64)(r 2^32) of the
// range's ends; W_max = W(d_max); G = ceil(W_max 2^32 / (hop d_min)), the callbacks an output block
// waits; latency = (G + 1) hop; K >= W_max (a multiple of 4): the row's history samples; row_len:
// floats of a channel's scratch row, K + ceil((G + max_nframes) hop d_max / 2^32) + hop + 4 rounded
// up to a multiple of 4 (the final samples a push can leave behind the history);
// ring_cap = G + max_nframes steps.  false: hop or max_nframes < 1, a quality other than 0, 1, a
// range with a NaN, outside [1/4, 4] or with ratio_min > ratio_max, (G + max_nframes) hop >= 2^28.
struct RtPitchmapPlan {
    long long d_min, d_max;
    int W_max, G, latency, K;
    long long row_len, ring_cap;
};
bool rt_pitchmap_plan(int hop, int quality, float ratio_min, float ratio_max, int max_nframes, RtPitchmapPlan* out);
// ---- real-time harmoniser (pv_rt_harmonizer_*): the most voices per channel at
// this n_samps (a wave per voice in one workgroup, its LDS the bound: 8, 8, 8, 4 for 256 .. 2048), 0
// where there is no kernel.  Every voice plans as rt_pitchmap_plan.
int rt_harmonizer_max_voices(int n_samps);

// ---- pitch correction (pv_pitch_correct_plan): track [frames] {f0, strength}
// -> ratio [n], one per output frame (pos: its analysis position, nullptr: u); false on a bad
// argument (cfg's ranges, a position that is not finite, frames or n < 1)
bool pitch_correct_plan(const pv_float2* track, int frames, const double* pos, int n, const pv_pitch_correct& cfg,
                        double* ratio);

}  // namespace pvtab
#pragma GCC visibility pop
