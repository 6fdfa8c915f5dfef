// pv_tables.cpp — pure-host recipes of libpv (pv_tables.hpp): no HIP header, no device call.
#include "pv_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace pvtab {

bool is_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

// ---- table recipes (identical double -> float formulas to the oracle, pvref.c) ----
void hann_periodic(int N, std::vector<float>& w) {
    w.resize(N);
    for (int n = 0; n < N; ++n)
        w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * (double)n / (double)N));
}

void hann_ref(int N, std::vector<float>& w) {
    // phaseVocoder.h:64-66 (1-argument constructor): 0.5f * (1.f - cosf(2.f*M_PI*i / samples));
    // 2.f*M_PI*i/samples is evaluated in double and rounded to float for cosf
    w.resize(N);
    for (int i = 0; i < N; ++i) w[i] = 0.5f * (1.f - cosf((float)(2.0 * kPi * (double)i / (double)N)));
}

void hamming_ref(int N, std::vector<float>& w) {
    // phaseVocoder.h:85-89
    w.resize(N);
    float omega = (float)(2.0 * kPi / (double)(N - 1));
    for (int i = 0; i < N; ++i) {
        float arg = omega * (float)i;
        w[i] = 0.54f - 0.46f * cosf(arg);
    }
}

void std_gain(int N, int hs, std::vector<float>& gain) {
    gain.resize(N);
    double sw2 = 0.0;
    std::vector<double> wd(N);
    for (int i = 0; i < N; ++i) {
        wd[i] = 0.5 - 0.5 * std::cos(2.0 * kPi * (double)i / (double)N);
        sw2 += wd[i] * wd[i];
    }
    for (int i = 0; i < N; ++i) gain[i] = (float)(wd[i] * ((double)hs / sw2) / (double)N);
}

void compat_gain(const std::vector<float>& win, std::vector<float>& gain) {
    const int N = (int)win.size();
    gain.resize(N);
    for (int i = 0; i < N; ++i) gain[i] = win[i] / (float)N;  // kernel.cu:380 /N, :406 window
}

pv_float2 tw_entry(long long m, long long L) {
    double a = 2.0 * kPi * (double)m / (double)L;
    return pv_float2{(float)std::cos(a), (float)(-std::sin(a))};
}

// stage-major table for an L-point Stockham FFT: stage Ns at [Ns-1, 2Ns-1)
void stage_twiddles(int L, std::vector<pv_float2>& t) {
    t.assign(L, pv_float2{0.f, 0.f});
    for (int Ns = 1; Ns < L; Ns <<= 1)
        for (int idx = 0; idx < Ns; ++idx) t[Ns - 1 + idx] = tw_entry((long long)idx * (L / (2 * Ns)), L);
}

// The FFT table of an L-point transform: the contract-v3 pass table for L in [128, 512]
// (pass P >= 1: S rows of R - 1 entries e^{-2 pi i m q/(R S)}, the oracle's
// pvr_fft_v3_table), the stage-major radix-2 table otherwise; L entries either way.  v3: the
// pass table at any L (the batched synthesis's L = 1024 inverse FFT, which no contract binds).
void fft_table(int L, std::vector<pv_float2>& t, bool v3) {
    if (!v3 && (L < 128 || L > 512)) {
        stage_twiddles(L, t);
        return;
    }
    t.assign(L, pv_float2{0.f, 0.f});
    const int E = L / 64;
    int off = 0;
    for (int S = E; S < L;) {
        const int R = std::min(E, L / S);
        for (int m = 0; m < S; ++m)
            for (int q = 1; q < R; ++q)
                t[off + m * (R - 1) + (q - 1)] = tw_entry(((long long)m * q * (L / (R * S))) % L, L);
        off += S * (R - 1);
        S *= R;
    }
}

// d_tw_syn: the synthesis-side L-point table (stage-major or v3, fft_table), then at L = 1024
// the v3 pass table of the batched synthesis's inverse FFT (k_synthesis reads tw + L; the
// real-time and fused kernels run the analysis transform from the first table too), at
// L = 256, 512 the L/2-point table of the fused pitch-2 resynthesis (k_fused MODE 4, tw + L;
// the single launch exists for L <= 512 only)
int tw_syn_len(int L) { return L == 1024 ? 2 * L : (L == 256 || L == 512) ? L + L / 2 : L; }

void tw_syn_table(int L, std::vector<pv_float2>& t) {
    fft_table(L, t);
    if (L == 1024) {
        std::vector<pv_float2> t3;
        fft_table(L, t3, true);
        t.insert(t.end(), t3.begin(), t3.end());
    } else if (tw_syn_len(L) > L) {
        std::vector<pv_float2> th;
        fft_table(L / 2, th);
        t.insert(t.end(), th.begin(), th.end());
    }
}

void split_twiddles(int N, std::vector<pv_float2>& t) {
    t.resize(N / 2 + 1);
    for (int k = 0; k <= N / 2; ++k) t[k] = tw_entry(k, N);
}

Geometry geometry(int N, int hop_div, int mode, int effect, float scale) {
    Geometry g{};
    g.hop = N / hop_div;  // phaseVocoder.h:79
    if (effect == PV_TIME_SHIFT) {
        float f = scale * (float)g.hop;  // phaseVocoder.h:104 (float -> int)
        g.hs = (int)f;
    } else {
        g.hs = g.hop;  // PITCH_SHIFT: defined by the build (reference leaves it unset)
    }
    g.pitch = (mode == PV_MODE_STANDARD && effect == PV_PITCH_SHIFT) ? 1 : 0;
    g.L_syn = N / 2;
    g.L_ana = (mode == PV_MODE_STANDARD) ? N / 2 : N;
    g.bins = N / 2 + 1;
    g.bins_pad = (g.bins + 7) & ~7;
    g.tail_len = N - g.hs;
    return g;
}

void phase_tables(int N, const Geometry& g, float scale, PhaseTables& t) {
    const int B = g.bins;
    t.ek.resize(B);
    t.jk.resize(B);
    for (int k = 0; k < B; ++k) {
        long long kh = (long long)k * g.hop;
        long long r = kh % N;
        long long rr = (r > N / 2) ? r - N : r;
        t.ek[k] = (float)(2.0 * kPi * (double)rr / (double)N);
        t.jk[k] = (kh - rr) / N;
    }
    unsigned long long pn = 1, qd = 1;
    if (g.pitch) {
        int e2 = 0;
        double m = std::frexp((double)scale, &e2);      // scale = m * 2^e2, m in [0.5,1)
        long long mant = (long long)std::ldexp(m, 24);  // exact: float has 24 bits
        int ex = e2 - 24;
        while ((mant & 1) == 0 && ex < 0) { mant >>= 1; ++ex; }
        if (ex >= 0) { pn = (unsigned long long)mant << ex; qd = 1; }
        else { pn = (unsigned long long)mant; qd = 1ull << (-ex); }
        t.rho = scale;
    } else {
        long long a = g.hs, b = g.hop;
        long long x = a, y = b;
        while (y) { long long tt = x % y; x = y; y = tt; }
        pn = a / x;
        qd = b / x;
        t.rho = (float)((double)g.hs / (double)g.hop);
    }
    t.p = pn;
    t.q = qd;
    t.p_mod = pn % qd;
    t.q_pow2 = is_pow2((long long)qd) ? 1 : 0;
    t.inv_q = (float)(1.0 / (double)qd);
    t.jk_mod.resize(B);
    for (int k = 0; k < B; ++k) {
        unsigned long long v = ((pn % qd) * ((unsigned long long)t.jk[k] % qd)) % qd;
        t.jk_mod[k] = (unsigned)v;
    }
}

bool bins_repeat_mod64(const PhaseTables& t) {
    const int B = (int)t.ek.size();
    bool kl = B > 64 && t.ek[B - 1] == t.ek[0];
    for (int k = 64; kl && k < B - 1; ++k) kl = (t.ek[k] == t.ek[k & 63]) && (t.jk_mod[k] == t.jk_mod[k & 63]);
    return kl;
}

void pitch_map(int bins, bool pitch, float scale, PitchMap& m) {
    const int B = bins;
    m.first.assign(B, -1);
    m.cnt.assign(B, 0);
    if (pitch) {
        const double beta = (double)scale;
        for (int k = 0; k < B; ++k) {
            long long kp = (long long)std::floor(beta * (double)k + 0.5);
            if (kp < 0 || kp >= B) continue;
            if (m.first[kp] < 0) m.first[kp] = k;
            m.cnt[kp]++;
        }
    }
    m.src_hi = B - 1;
    if (pitch) {
        m.src_hi = -1;
        for (int k = 0; k < B; ++k)
            if (m.cnt[k] > 0) m.src_hi = std::max(m.src_hi, m.first[k] + m.cnt[k] - 1);
    }
}

// warp position of bin k after the P:Q resampling of the stretched signal, in exact integers:
// a = k out_hop, i_k = a div hop, f_k = (a mod hop) / hop (the fp32 nearest: both are exact in
// fp32 and the division is correctly rounded); from the first bin with i_k >= L on, {L, 0}
void warp_map(int bins, int hop, int out_hop, std::vector<int>& idx, std::vector<float>& frac) {
    const int L = bins - 1;
    idx.assign(bins, L);
    frac.assign(bins, 0.0f);
    for (int k = 0; k < bins; ++k) {
        const long long a = (long long)k * out_hop;
        const long long i = a / hop, r = a % hop;
        if (i >= L) continue;
        idx[k] = (int)i;
        frac[k] = (float)r / (float)hop;
    }
}

// the time map's split (pv_timemap_split): i = floor(pos), a = fp32(pos - i)
// (the difference is exact in fp64; a may round up to 1)
bool timemap_split(const double* pos, int n, int* idx, float* frac) {
    for (int u = 0; u < n; ++u) {
        const double x = pos[u];
        if (!std::isfinite(x) || x < 0.0 || x >= 1073741824.0) return false;
        const double fl = std::floor(x);
        idx[u] = (int)fl;
        frac[u] = (float)(x - fl);
    }
    return true;
}

EnvOverrides read_env_overrides() {
    EnvOverrides e;
    // the single-launch and REF_COMPAT overrides (pv.h)
    if (const char* ev = std::getenv("PV_COMPAT_ANA_FRAMES")) {
        const int f = std::atoi(ev);
        if (f >= 1 && f <= 256) e.compat_ana_frames = f;
    }
    if (const char* eh = std::getenv("PV_FUSED_HALF")) e.fused_half = (eh[0] == '0') ? 0 : 1;
    if (const char* eb = std::getenv("PV_FUSED_BALANCE")) e.fused_balance = (eb[0] == '0') ? 0 : 1;
    if (const char* ev = std::getenv("PV_RUN_FRAMES")) e.run_frames = std::atoi(ev);
    if (const char* ev = std::getenv("PV_FUSED_FRAMES")) e.fused_frames = std::atoi(ev);
    if (const char* en = std::getenv("PV_FUSED")) e.fused = (en[0] == '0') ? 0 : 1;
    if (const char* ev = std::getenv("PV_SYN_LANEK")) e.syn_lanek = (ev[0] == '0') ? 0 : 1;
    // (anything but exactly "0" or "1" counts as unset)
    if (const char* ev = std::getenv("PV_RESIDENT"))
        e.resident = (ev[0] == '0' && ev[1] == 0) ? 0 : (ev[0] == '1' && ev[1] == 0) ? 1 : -1;
    return e;
}

// frames per wave-run before the round fit: longer runs amortise the halo frame each run
// transforms (1/F of the analysis work) as long as the batch still yields >= 2048 workgroups
// of 4 runs
static int base_run_frames(long long work, int L_syn) {
    // (measured on config 3: F = 32 / 48 / 64 / 96 -> 3.64 / 3.74 / 3.72 / 3.62e8 frames/s)
    int F = (work >= 2048LL * 4 * 48) ? 48 : (work >= 2048LL * 4 * 32) ? 32 : (work >= 1024LL * 4 * 16) ? 16 : 8;
    // a frame at L >= 1024 is twice the work: runs of 32 (measured on the config-4 slice,
    // 1024 channels x 861 frames: F = 24 / 32 / 40 / 48 / 64 -> 1.51-1.52 / 1.53-1.54 /
    // 1.47-1.48 / 1.49-1.50 / 1.46-1.49e8 frames/s)
    if (L_syn >= 1024 && F > 32) F = 32;
    return F;
}

bool run_fit_applies(long long work, int L_syn, int L_ana, int mode) {
    return base_run_frames(work, L_syn) == 48 && L_ana <= 512 && mode == PV_MODE_STANDARD;
}

int choose_run_frames(long long work, int L_syn, int L_ana, int mode, int wgs_per_cu, int waves_per_wg,
                      long long C, long long T, int hs, int tail_len, const EnvOverrides& env) {
    int F = base_run_frames(work, L_syn);
    // Large STANDARD batches at L <= 512: the analysis grid runs in rounds of (workgroups one
    // CU holds) x CUs, and a last partial round leaves most of the chip idle while its runs
    // finish.  Among F = 48, 56, .. 96 take the one with the fewest frame-times, rounds x F
    // (near-ties: the longer runs, below).  Config 3 at round 5's 5 workgroups per CU: 48 gives
    // 9216 workgroups = 8 rounds (the last a fifth full) x 48 = 384, 88 gives 5120 = 4 x 88 =
    // 352 (measured on two boxes: +1.7 / +1.8 % frames/s, profiles/r04_ab_c3_F.txt; what the
    // longer runs buy is the carry, seam and synthesis time — the analysis kernel itself is
    // within +-2 % from F = 24 to 88, profiles/r05_ab_c3_F_sweep.txt).  The rounds are counted
    // on the MI355X's 256 CUs whatever device the handle is on, and the workgroups per CU
    // come from the compiled kernel's resources: F, which sets where the overlap-add sums are
    // split into run seams (their rounding, <= 1e-6), depends only on the configuration, so
    // the same batch gives the same output bits on any gfx950 device or partition mode.
    if (run_fit_applies(work, L_syn, L_ana, mode) && wgs_per_cu > 0) {
        const int W = waves_per_wg;
        const long long slots = (long long)kRoundCUs * wgs_per_cu;
        // (round 6: the longest run within 2 % of the fewest frame-times — each run costs a
        // record, a carry and a seam; with the 4-wave/SIMD analysis config 3 has 48 -> 432
        // and 88 -> 440 frame-times, and F = 88 measured +1.9 % frames/s over 48)
        long long best = -1;
        long long cost_of[7];
        for (int j = 0, f = 48; f <= 96; f += 8, ++j) {
            const long long wgs = C * (((T + f - 1) / f + W - 1) / W);
            cost_of[j] = ((wgs + slots - 1) / slots) * f;
            if (best < 0 || cost_of[j] < best) best = cost_of[j];
        }
        for (int j = 0, f = 48; f <= 96; f += 8, ++j)
            if (cost_of[j] * 100 <= best * 102) F = f;
    }
    // tuning override (even, 8..256): PV_RUN_FRAMES
    {
        const int f = env.run_frames;
        if (f >= 8 && f <= 256 && f % 2 == 0) F = f;
    }
    // a run's output span must cover the overlap tail
    while ((long long)F * hs < tail_len) F += 4;
    return F;
}

// single-launch path (q = 1): no halo frame, so runs can be as short as the overlap tail
// allows (F hs >= N - hs) to give a single stream enough waves; PV_FUSED=0 disables it
// (tests compare both paths), PV_FUSED_FRAMES overrides its run length
int choose_fused_frames(int F, long long work, int hs, int tail_len, const EnvOverrides& env) {
    const int fmin = std::max(2, (tail_len + hs - 1) / hs);
    int Ff = (int)std::min<long long>(F, std::max<long long>(fmin, work / 4096));
    {
        const int f = env.fused_frames;
        if (f >= fmin && f <= 256) Ff = f;
    }
    return env.fused ? Ff : 0;
}

// a stream whose workgroups do not fill whole rounds of the 256 CUs (config 2: 862 =
// 3 x 256 + 94, so 94 CUs ran a 4th workgroup, 12 frames on their SIMDs against 9):
// exactly `rounds` workgroups per CU, some runs one frame longer (k_fused "balanced";
// PV_FUSED_BALANCE=0 turns it off).  The run boundaries move, so the seams' rounding
// does (<= 1e-6); the output depends only on the configuration.
void fused_rounds(int frames, int F, bool balance, int* nwg, int* n4) {
    const int nruns = (frames + F - 1) / F;
    *nwg = (nruns + 3) / 4;
    *n4 = 0;
    const int rounds = *nwg / kRoundCUs;
    // (decided from the frame count alone, for any number of channels: a channel's runs
    // and so its output bits are the same alone or in a batch — ADVICE r5)
    if (balance && rounds >= 1 && *nwg % kRoundCUs != 0) {
        const int G = rounds * kRoundCUs;
        const long long m = (long long)frames - 4LL * F * G;
        if (m > 0 && m <= 4LL * G) {
            *nwg = G;
            *n4 = (int)m;
        }
    }
}

bool resident_supported(const ResidentGeometry& g) {
    return g.mode == PV_MODE_STANDARD && !g.pitch && g.L_ana == 512 && g.L_syn == 512 && g.hop == 256 &&
           g.hs == 128 && g.q_pow2 && g.q >= 2 && g.q <= 4096 && g.k_lane &&
           (long long)g.F * g.hs >= g.tail_len;
}

int resident_min_channels(bool supported, const EnvOverrides& env) {
    if (!supported || env.resident == 0) return 0;
    return env.resident == 1 ? 1 : kResidentAutoChannels;
}

// ---- resampler
// {Z, rolloff, Kaiser beta} of the quality presets (include/pv.h)
static const double kResamplePresets[2][3] = {{16.0, 0.85, 8.555504641634386},
                                              {64.0, 0.9475937167399596, 14.769656459379492}};

// modified Bessel function I0 by its power series sum_k ((x / 2)^k / k!)^2
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

long long gcd_ll(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// half width W = ceil(Z / s) of the reduced ratio's filter (include/pv.h)
int resample_half_width(int P, int Q, int quality) {
    const double s = kResamplePresets[quality][1] * std::min(1.0, (double)Q / (double)P);
    return (int)std::ceil(kResamplePresets[quality][0] / s);
}

// the coefficients of phase r: row[t] = h(t - W + 1 - r / Q), t < 2W, fp64 rounded to fp32 once
void resample_row(int P, int Q, int quality, int W, int r, float* row) {
    const double Z = kResamplePresets[quality][0], rolloff = kResamplePresets[quality][1],
                 beta = kResamplePresets[quality][2];
    const double s = rolloff * std::min(1.0, (double)Q / (double)P);
    const double i0b = bessel_i0(beta);
    for (int t = 0; t < 2 * W; ++t) {
        const double tau = (double)(t - W + 1) - (double)r / (double)Q;
        const double u = s * tau / Z;
        double v = 0.0;
        if (std::fabs(u) < 1.0) {
            const double a = kPi * s * tau;
            const double sinc = (a == 0.0) ? 1.0 : std::sin(a) / a;
            v = s * sinc * bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
        }
        row[t] = (float)v;
    }
}

long long resample_length(int P, int Q, long long n_in) {
    if (n_in <= 0) return 0;
    return (n_in * Q + P - 1) / P;
}

// ---- variable-rate resampler (pv_varresample_*)
bool varresample_steps(const double* ratio, int n, long long* step) {
    for (int k = 0; k < n; ++k) {
        const double r = ratio[k];
        if (!std::isfinite(r) || r < 0.25 || r > 4.0) return false;
        step[k] = std::llrint(r * 4294967296.0);
    }
    return true;
}

// Sq: the largest even integer <= rolloff min(1, 2^32 / d) 2^32; W = ceil(Z / (Sq / 2^32))
void var_block_filter(long long d, int quality, unsigned* Sq, int* W) {
    const double v = kResamplePresets[quality][1] * std::min(1.0, 4294967296.0 / (double)d) * 4294967296.0;
    const unsigned sq = (unsigned)std::floor(v) & ~1u;
    *Sq = sq;
    *W = (int)std::ceil(kResamplePresets[quality][0] / ((double)sq / 4294967296.0));
}

double resample_zero_crossings(int quality) { return kResamplePresets[quality][0]; }
double resample_rolloff(int quality) { return kResamplePresets[quality][1]; }

// the Kaiser window over u = i / n with the sinc's 1 / pi: {w(u_i) / pi, the rise to the next
// entry} for i < n (each value rounded to fp32 first: the interpolation ends on the next entry),
// then {0, 0} up to `len` entries
void var_window_table(int quality, int n, int len, std::vector<float>& tab) {
    const double beta = kResamplePresets[quality][2], i0b = bessel_i0(beta);
    std::vector<float> w(n + 1);
    for (int i = 0; i <= n; ++i) {
        const double u = (double)i / (double)n;
        w[i] = (float)(bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b / kPi);
    }
    tab.assign(2 * (size_t)len, 0.0f);
    for (int i = 0; i < n; ++i) {
        tab[2 * i] = w[i];
        tab[2 * i + 1] = w[i + 1] - w[i];
    }
}

// The real-time pitch map's latency and buffer sizes (integers; the steps are exact: an fp32 at or
// above 1/4 is a multiple of 2^-26)
int rt_harmonizer_max_voices(int n_samps) {
    return (n_samps == 256 || n_samps == 512 || n_samps == 1024) ? 8 : (n_samps == 2048) ? 4 : 0;
}

bool rt_pitchmap_plan(int hop, int quality, float ratio_min, float ratio_max, int max_nframes, RtPitchmapPlan* out) {
    if (hop < 1 || max_nframes < 1 || (quality != 0 && quality != 1)) return false;
    if (!(ratio_min >= 0.25f) || !(ratio_max <= 4.0f) || !(ratio_min <= ratio_max)) return false;
    RtPitchmapPlan p{};
    p.d_min = (long long)(ratio_min * 0x1p32f);
    p.d_max = (long long)(ratio_max * 0x1p32f);
    unsigned sq;
    var_block_filter(p.d_max, quality, &sq, &p.W_max);
    const long long den = (long long)hop * p.d_min;
    p.G = (int)((((long long)p.W_max << 32) + den - 1) / den);
    p.latency = (p.G + 1) * hop;
    p.K = (p.W_max + 3) & ~3;
    // ((G + max_nframes) hop < 2^28 and d_max <= 2^34: the product stays below 2^62)
    if ((long long)(p.G + (long long)max_nframes) * hop >= (1LL << 28)) return false;
    const long long span = ((long long)(p.G + max_nframes) * hop * p.d_max + kVarOne - 1) >> 32;
    p.row_len = (p.K + span + hop + 4 + 3) & ~3LL;
    p.ring_cap = (long long)p.G + max_nframes;
    *out = p;
    return true;
}

// The pitch map's plan (pv_pitchmap_plan): the time map of the stretch and the steps of the
// resampling after it.  Integers and fp64 only.
bool pitchmap_plan(int N, int hop, const double* pos, const double* ratio, int n, std::vector<double>& pos_s,
                   std::vector<long long>& step) {
    if (n < 1 || hop < 1 || N < hop || (long long)n * hop >= (1LL << 28)) return false;
    for (int u = 0; u < n; ++u)
        if (!std::isfinite(pos[u]) || pos[u] < 0.0 || pos[u] >= 1073741824.0) return false;
    const long long L = (long long)n * hop + N - hop;
    const long long nb = (L + hop - 1) / hop;
    step.assign((size_t)nb, 0);
    if (!varresample_steps(ratio, n, step.data())) return false;
    for (long long b = n; b < nb; ++b) step[(size_t)b] = step[(size_t)n - 1];
    std::vector<long long> S((size_t)n + 1, 0);  // Sigma_0 .. Sigma_n < 2^28 2^34 = 2^62
    for (int b = 0; b < n; ++b) S[b + 1] = S[b] + (long long)hop * step[b];
    const long long unit = (long long)hop << 32;
    const long long n_s = std::max(1LL, (S[n] + unit - 1) / unit);
    pos_s.assign((size_t)n_s, 0.0);
    int b = 0;
    for (long long v = 0; v < n_s; ++v) {
        const long long t = v * unit;
        while (b < n - 1 && t >= S[b + 1]) ++b;
        const double w = (double)(t - S[b]) / (double)(S[b + 1] - S[b]);
        const double p0 = pos[b], p1 = pos[std::min(b + 1, n - 1)];
        pos_s[(size_t)v] = p0 + w * (p1 - p0);
    }
    return true;
}

// The correction curve of a pitch track (pv_pitch_correct_plan): every voiced
// frame's distance to the nearest allowed semitone (the lower one on a tie), held over the
// unvoiced frames, through a one-pole smoother, as a pitch ratio per output frame.  fp64 only.
bool pitch_correct_plan(const pv_float2* track, int frames, const double* pos, int n, const pv_pitch_correct& cfg,
                        double* ratio) {
    if (frames < 1 || n < 1) return false;
    if (!(cfg.a4 > 0.0) || !std::isfinite(cfg.a4)) return false;
    if (cfg.scale_mask == 0u || cfg.scale_mask >= 4096u) return false;
    if (std::isnan(cfg.strength_min)) return false;
    if (!(cfg.retune > 0.0 && cfg.retune <= 1.0)) return false;
    if (pos)
        for (int u = 0; u < n; ++u)
            if (!std::isfinite(pos[u])) return false;
    auto allowed = [&](long long m) { return (cfg.scale_mask >> (unsigned)(((m % 12) + 12) % 12)) & 1u; };
    double s = 0.0;
    for (int u = 0; u < n; ++u) {
        const double x = std::floor((pos ? pos[u] : (double)u) + 0.5);
        const int t = x <= 0.0 ? 0 : x >= (double)(frames - 1) ? frames - 1 : (int)x;
        const double f0 = (double)track[t].x;
        double c = s;
        // (a NaN fails every comparison: unvoiced; so is a frame whose note is not finite, f0 / a4
        // beyond the doubles)
        const bool voiced = std::isfinite(f0) && f0 > 0.0 && (double)track[t].y >= cfg.strength_min;
        const double note = voiced ? 69.0 + 12.0 * std::log2(f0 / cfg.a4) : 0.0;
        if (voiced && std::isfinite(note)) {
            long long lo = (long long)std::floor(note), hi = (long long)std::ceil(note);
            while (!allowed(lo)) --lo;  // (at most 11 steps each: the mask is not empty)
            while (!allowed(hi)) ++hi;
            const double target = (note - (double)lo <= (double)hi - note) ? (double)lo : (double)hi;
            c = (target - note) / 12.0;
        }
        s = s + cfg.retune * (c - s);
        ratio[u] = std::min(4.0, std::max(0.25, std::exp2(s)));
    }
    return true;
}

}  // namespace pvtab
