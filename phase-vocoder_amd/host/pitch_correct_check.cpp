// pitch_correct_check — the pitch-correction planner (pvtab::pitch_correct_plan, pv_tables.cpp;
// DESIGN.md §3.14) in a program of its own: plain host C++, no HIP, no GPU.  Built by the plain
// host compiler, and under AddressSanitizer and UBSan (make pitch-correct-san;
// tests/test_pitchtrack_ref.py runs both).  Exact-size heap buffers, so that a read or a write
// past either end is caught; positions far outside the track, non-finite tracks, every refusal.
// Prints the ratios of the first case, one "%.17g" per line, then "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../csrc/pv_tables.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

pv_pitch_correct config(double a4, unsigned mask, double smin, double retune) {
    pv_pitch_correct c{};
    c.abi_version = PV_ABI_VERSION;
    c.a4 = a4;
    c.scale_mask = mask;
    c.strength_min = smin;
    c.retune = retune;
    return c;
}

}  // namespace

int main() {
    const double a4 = 440.0 / 44100.0;
    const unsigned major = 0xAB5u;  // C D E F G A B
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // 30 cents under A4, a few unvoiced and non-finite frames, retune 0.5
    {
        const int frames = 9, n = 12;
        std::vector<pv_float2> track((size_t)frames);
        for (int t = 0; t < frames; ++t) track[(size_t)t] = pv_float2{(float)(a4 * std::exp2(-0.3 / 12.0)), 0.9f};
        track[2] = pv_float2{0.0f, 0.0f};
        track[3] = pv_float2{(float)nan, 0.9f};
        track[4] = pv_float2{(float)inf, 0.9f};
        track[5] = pv_float2{-0.01f, 0.9f};
        track[6] = pv_float2{0.01f, (float)nan};
        track[7] = pv_float2{1e-45f, 0.9f};
        std::vector<double> ratio((size_t)n, -1.0);
        expect(pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, major, 0.5, 0.5), ratio.data()),
               "plan, identity positions");
        for (double r : ratio) {
            expect(r >= 0.25 && r <= 4.0, "ratio in [1/4, 4]");
            std::printf("%.17g\n", r);
        }
        // positions below, inside, above and far outside the track
        std::vector<double> pos{-1e300, -0.6, 0.49, 0.5, 7.5, 8.49, 8.5, 1e9, 1e300, 3.0, 2.0, 1.0};
        expect(pvtab::pitch_correct_plan(track.data(), frames, pos.data(), n, config(a4, 1u << 9, 0.5, 1.0), ratio.data()),
               "plan, positions");
        // a tiny and a huge a4: the note leaves every table, the ratio stays clamped
        expect(pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(5e-324, 1u, 0.0, 1.0), ratio.data()),
               "plan, denormal a4");
        expect(pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(1e300, 1u << 11, -inf, 1.0), ratio.data()),
               "plan, huge a4");
        for (double r : ratio) expect(r >= 0.25 && r <= 4.0, "ratio in [1/4, 4] (huge a4)");

        // refusals
        const pv_pitch_correct good = config(a4, major, 0.5, 1.0);
        expect(!pvtab::pitch_correct_plan(track.data(), 0, nullptr, n, good, ratio.data()), "frames 0");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, 0, good, ratio.data()), "n 0");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(0.0, major, 0.5, 1.0), ratio.data()), "a4 0");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(nan, major, 0.5, 1.0), ratio.data()), "a4 NaN");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(inf, major, 0.5, 1.0), ratio.data()), "a4 inf");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, 0u, 0.5, 1.0), ratio.data()), "mask 0");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, 4096u, 0.5, 1.0), ratio.data()), "mask 2^12");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, major, nan, 1.0), ratio.data()), "strength NaN");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, major, 0.5, 0.0), ratio.data()), "retune 0");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, major, 0.5, 1.5), ratio.data()), "retune 1.5");
        expect(!pvtab::pitch_correct_plan(track.data(), frames, nullptr, n, config(a4, major, 0.5, nan), ratio.data()), "retune NaN");
        pos[4] = nan;
        expect(!pvtab::pitch_correct_plan(track.data(), frames, pos.data(), n, good, ratio.data()), "position NaN");
    }
    // one frame, one output
    {
        std::vector<pv_float2> track(1, pv_float2{(float)(a4 * 2.0), 1.0f});
        std::vector<double> ratio(1, -1.0);
        // A5 = note 81 between the allowed G#5 and A#5: the lower one, a semitone down
        expect(pvtab::pitch_correct_plan(track.data(), 1, nullptr, 1, config((double)(float)a4, (1u << 8) | (1u << 10), 0.5, 1.0),
                                         ratio.data()), "plan, one frame");
        expect(std::fabs(ratio[0] - std::exp2(-1.0 / 12.0)) < 1e-15, "a tie goes to the lower note");
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
