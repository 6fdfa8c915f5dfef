// tables_dump — the host-side tables and choices of libpv (csrc/pv_tables.cpp), written out
// for comparison with the oracle.  Links pv_tables.cpp only: no GPU, no HIP.
//
//   tables_dump N hop_div mode effect scale window [file]
//       mode 0 = REF_COMPAT, 1 = STANDARD; effect t | p; window as pv_config.window.
//       Raw little-endian arrays, in this order (B = N/2 + 1):
//         int64  head[16]  N, hop, out hop, L_ana, L_syn, B, p, q, p mod q, q_pow2, src_hi,
//                          bins_repeat_mod64, bits of rho (float), bits of 1/q (float), 0, 0
//         float  win[N], gain[N]
//         float2 tw_ana[L_ana], tws_ana[L_ana + 1], tw_syn[tw_syn_len(L_syn)], tws_syn[N/2 + 1]
//         float  ek[B];  int64 jk[B];  uint32 jk_mod[B];  int32 src_first[B], src_cnt[B]
//   tables_dump resample P Q quality [file]
//       int64 head[4]  reduced P, reduced Q, quality, W;  then float row[Q][2W]
//   tables_dump warp N hop out_hop [file]
//       the envelope warp map (pv_pitch_set_formant): int32 idx[N/2 + 1], then float frac[N/2 + 1]
//   tables_dump choose C T N hop_div mode effect scale wgs_per_cu waves_per_wg
//       prints "F Ff": frames per run, and per run of the single launch (environment
//       overrides apply, as in pv_create)
//   tables_dump balance frames F
//       prints "nwg n4": the single launch's workgroups and its runs one frame longer
//   tables_dump resident mode pitch L_ana L_syn hop hs q_pow2 q k_lane F tail_len
//       prints "supported threshold": resident_supported of the geometry and, with PV_RESIDENT
//       from the environment, resident_min_channels
//   tables_dump rtpitchmap hop quality ratio_min ratio_max max_nframes
//       prints "d_min d_max W_max G latency K row_len ring_cap": the real-time pitch map's plan
//       (pv_rt_pitchmap_reserve; the ratios as strtof reads them, hexadecimal floats included), or
//       "refused"
// [file] absent or "-": stdout.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../csrc/pv_tables.hpp"

using namespace pvtab;

namespace {

template <typename T>
void put(FILE* f, const T* p, size_t n) {
    if (n && std::fwrite(p, sizeof(T), n, f) != n) {
        std::perror("tables_dump: write");
        std::exit(1);
    }
}
template <typename T>
void put(FILE* f, const std::vector<T>& v) { put(f, v.data(), v.size()); }

int64_t float_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return (int64_t)u;
}

FILE* open_out(int argc, char** argv, int idx) {
    if (idx >= argc || std::strcmp(argv[idx], "-") == 0) return stdout;
    FILE* f = std::fopen(argv[idx], "wb");
    if (!f) {
        std::perror(argv[idx]);
        std::exit(1);
    }
    return f;
}

int usage() {
    std::fprintf(stderr,
                 "usage: tables_dump N hop_div mode effect scale window [file]\n"
                 "       tables_dump resample P Q quality [file]\n"
                 "       tables_dump warp N hop out_hop [file]\n"
                 "       tables_dump choose C T N hop_div mode effect scale wgs_per_cu waves_per_wg\n"
                 "       tables_dump balance frames F\n"
                 "       tables_dump resident mode pitch L_ana L_syn hop hs q_pow2 q k_lane F tail_len\n"
                 "       tables_dump rtpitchmap hop quality ratio_min ratio_max max_nframes\n");
    return 2;
}

// the refusals of pv_create that keep the recipes inside their domain
bool config_ok(int N, int hop_div, int mode, int effect, float scale) {
    if (!is_pow2(N) || N < 256 || N > 2048 || hop_div <= 0 || N / hop_div <= 0) return false;
    if (mode != PV_MODE_STANDARD && mode != PV_MODE_REF_COMPAT) return false;
    if (effect != PV_TIME_SHIFT && effect != PV_PITCH_SHIFT) return false;
    return scale > 0.0f && scale <= 64.0f;
}

int dump_tables(int argc, char** argv) {
    if (argc < 7) return usage();
    const int N = std::atoi(argv[1]), hop_div = std::atoi(argv[2]), mode = std::atoi(argv[3]);
    const int effect = argv[4][0], window = std::atoi(argv[6]);
    const float scale = (float)std::atof(argv[5]);
    if (!config_ok(N, hop_div, mode, effect, scale)) return usage();
    const Geometry g = geometry(N, hop_div, mode, effect, scale);
    if (g.hs <= 0 || g.hs > N) return usage();
    PhaseTables pt;
    phase_tables(N, g, scale, pt);
    PitchMap pm;
    pitch_map(g.bins, g.pitch != 0, scale, pm);
    FILE* f = open_out(argc, argv, 7);
    const int64_t head[16] = {N, g.hop, g.hs, g.L_ana, g.L_syn, g.bins, (int64_t)pt.p, (int64_t)pt.q,
                              (int64_t)pt.p_mod, pt.q_pow2, pm.src_hi, bins_repeat_mod64(pt) ? 1 : 0,
                              float_bits(pt.rho), float_bits(pt.inv_q), 0, 0};
    put(f, head, 16);
    std::vector<float> win, gain;
    if (mode == PV_MODE_STANDARD) {
        hann_periodic(N, win);
        std_gain(N, g.hs, gain);
    } else {
        if (window == PV_WINDOW_HANN_REF) hann_ref(N, win);
        else hamming_ref(N, win);
        compat_gain(win, gain);
    }
    put(f, win);
    put(f, gain);
    std::vector<pv_float2> t;
    fft_table(g.L_ana, t);
    put(f, t);
    split_twiddles(2 * g.L_ana, t);
    put(f, t);
    tw_syn_table(g.L_syn, t);
    put(f, t);
    split_twiddles(N, t);
    put(f, t);
    put(f, pt.ek);
    std::vector<int64_t> jk(pt.jk.begin(), pt.jk.end());
    put(f, jk);
    put(f, pt.jk_mod);
    put(f, pm.first);
    put(f, pm.cnt);
    if (f != stdout) std::fclose(f);
    return 0;
}

int dump_resample(int argc, char** argv) {
    if (argc < 5) return usage();
    const int p = std::atoi(argv[2]), q = std::atoi(argv[3]), quality = std::atoi(argv[4]);
    if (p <= 0 || q <= 0 || (quality != 0 && quality != 1)) return usage();
    const long long gd = gcd_ll(p, q);
    const int P = (int)(p / gd), Q = (int)(q / gd);
    if (P > 4096 || Q > 4096 || P > 4 * Q || Q > 4 * P || P == Q) return usage();
    const int W = resample_half_width(P, Q, quality);
    FILE* f = open_out(argc, argv, 5);
    const int64_t head[4] = {P, Q, quality, W};
    put(f, head, 4);
    std::vector<float> row(2 * W);
    for (int r = 0; r < Q; ++r) {
        resample_row(P, Q, quality, W, r, row.data());
        put(f, row);
    }
    if (f != stdout) std::fclose(f);
    return 0;
}

int dump_warp(int argc, char** argv) {
    if (argc < 5) return usage();
    const int N = std::atoi(argv[2]), hop = std::atoi(argv[3]), hs = std::atoi(argv[4]);
    if (!is_pow2(N) || N < 256 || N > 2048 || hop <= 0 || hop > N || hs <= 0 || hs > N) return usage();
    std::vector<int> idx;
    std::vector<float> frac;
    warp_map(N / 2 + 1, hop, hs, idx, frac);
    FILE* f = open_out(argc, argv, 5);
    put(f, idx);
    put(f, frac);
    if (f != stdout) std::fclose(f);
    return 0;
}

int choose(int argc, char** argv) {
    if (argc < 11) return usage();
    const long long C = std::atoll(argv[2]), T = std::atoll(argv[3]);
    const int N = std::atoi(argv[4]), hop_div = std::atoi(argv[5]), mode = std::atoi(argv[6]);
    const int effect = argv[7][0];
    const float scale = (float)std::atof(argv[8]);
    const int wpc = std::atoi(argv[9]), W = std::atoi(argv[10]);
    if (C < 1 || T < 1 || W < 1 || !config_ok(N, hop_div, mode, effect, scale)) return usage();
    const Geometry g = geometry(N, hop_div, mode, effect, scale);
    if (g.hs <= 0 || g.hs > N) return usage();
    const EnvOverrides env = read_env_overrides();
    const long long work = C * T;
    const int F = choose_run_frames(work, g.L_syn, g.L_ana, mode, wpc, W, C, T, g.hs, g.tail_len, env);
    std::printf("%d %d\n", F, choose_fused_frames(F, work, g.hs, g.tail_len, env));
    return 0;
}

int balance(int argc, char** argv) {
    if (argc < 4) return usage();
    const int frames = std::atoi(argv[2]), F = std::atoi(argv[3]);
    if (frames < 1 || F < 1) return usage();
    int nwg = 0, n4 = 0;
    fused_rounds(frames, F, read_env_overrides().fused_balance != 0, &nwg, &n4);
    std::printf("%d %d\n", nwg, n4);
    return 0;
}

// resident mode pitch L_ana L_syn hop hs q_pow2 q k_lane F tail_len -> "supported threshold"
// (PV_RESIDENT from the environment)
int resident(int argc, char** argv) {
    if (argc < 13) return usage();
    ResidentGeometry g{};
    g.mode = std::atoi(argv[2]);
    g.pitch = std::atoi(argv[3]);
    g.L_ana = std::atoi(argv[4]);
    g.L_syn = std::atoi(argv[5]);
    g.hop = std::atoi(argv[6]);
    g.hs = std::atoi(argv[7]);
    g.q_pow2 = std::atoi(argv[8]);
    g.q = std::strtoull(argv[9], nullptr, 10);
    g.k_lane = std::atoi(argv[10]);
    g.F = std::atoi(argv[11]);
    g.tail_len = std::atoi(argv[12]);
    const bool ok = resident_supported(g);
    std::printf("%d %d\n", ok ? 1 : 0, resident_min_channels(ok, read_env_overrides()));
    return 0;
}

// rtpitchmap hop quality ratio_min ratio_max max_nframes -> the plan, or "refused"
int rtpitchmap(int argc, char** argv) {
    if (argc < 7) return usage();
    RtPitchmapPlan p{};
    if (!rt_pitchmap_plan(std::atoi(argv[2]), std::atoi(argv[3]), std::strtof(argv[4], nullptr),
                          std::strtof(argv[5], nullptr), std::atoi(argv[6]), &p)) {
        std::printf("refused\n");
        return 0;
    }
    std::printf("%lld %lld %d %d %d %d %lld %lld\n", p.d_min, p.d_max, p.W_max, p.G, p.latency, p.K, p.row_len,
                p.ring_cap);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    if (cmd == "resample") return dump_resample(argc, argv);
    if (cmd == "warp") return dump_warp(argc, argv);
    if (cmd == "choose") return choose(argc, argv);
    if (cmd == "balance") return balance(argc, argv);
    if (cmd == "resident") return resident(argc, argv);
    if (cmd == "rtpitchmap") return rtpitchmap(argc, argv);
    return dump_tables(argc, argv);
}
