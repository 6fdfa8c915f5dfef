// pv_api_misc.cpp — the stand-alone FFT and the harmoniser of libpv.
#include <map>
#include <mutex>

#include "pv_host.hpp"

using namespace pvhost;

// ---------------------------------------------------------------- standalone FFT
namespace {
std::mutex g_fft_mu;
std::map<std::pair<int, int>, float2*> g_fft_tw;  // (device, n) -> stage-major twiddles
}  // namespace

extern "C" pv_status pv_fft_c2c(const pv_float2* in, pv_float2* out, int n, int batch, int inverse,
                                void* stream) {
    if (!in || !out) return fail(PV_ERR_ARG, "null in/out");
    if (batch < 0) return fail(PV_ERR_ARG, "negative batch");
    if (!is_pow2(n) || n < 2 || n > 2048) return fail(PV_ERR_UNSUPPORTED, "fft size: power of two in [2, 2048]");
    if (batch == 0) return PV_OK;
    int dev = 0;
    PV_HIP(hipGetDevice(&dev));
    float2* tw = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_fft_mu);
        auto it = g_fft_tw.find({dev, n});
        if (it == g_fft_tw.end()) {
            std::vector<pv_float2> t;
            fft_table(n, t);
            static_assert(sizeof(pv_float2) == sizeof(float2), "host and device entries share a layout");
            DevBuf<float2> buf;
            PV_HIP(buf.upload(reinterpret_cast<const float2*>(t.data()), t.size()));
            tw = buf.p;
            buf.p = nullptr;  // cached for the life of the process
            g_fft_tw[{dev, n}] = tw;
        } else {
            tw = it->second;
        }
    }
    hipError_t e = pv::launch_fft(n, inverse ? 1 : 0, reinterpret_cast<const float2*>(in),
                                  reinterpret_cast<float2*>(out), tw, batch, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("fft launch: ") + hipGetErrorString(e));
    return PV_OK;
}

// ---------------------------------------------------------------- harmoniser
// README.md:50 "harmonization of input signals (i.e. multiple pitch shifts on a single
// input)": one analysis + one unwrap scan, then one synthesis per voice (its own pitch
// map and output-phase ratio), optionally mixed.
struct pv_harmonizer {
    std::vector<pv_handle*> voices;
};

extern "C" {

void pv_harmonizer_destroy(pv_harmonizer* hz) {
    if (!hz) return;
    for (pv_handle* v : hz->voices) pv_destroy(v);
    delete hz;
}

pv_status pv_harmonizer_create(const pv_config* cfg, const float* ratios, int voices, pv_harmonizer** out) {
    if (!cfg || !ratios || !out) return fail(PV_ERR_ARG, "null argument");
    // the version first: no other field of a caller's struct is read before it matches
    pv_status st = check_abi(cfg);
    if (st != PV_OK) return st;
    if (cfg->tables_external) return fail(PV_ERR_UNSUPPORTED, "tables_external: batch handles only");
    *out = nullptr;
    if (voices <= 0 || voices > 64) return fail(PV_ERR_ARG, "voices must be in [1, 64]");
    if (cfg->mode != PV_MODE_STANDARD) return fail(PV_ERR_UNSUPPORTED, "the harmoniser runs the STANDARD pipeline");
    pv_harmonizer* hz = new pv_harmonizer();
    for (int k = 0; k < voices; ++k) {
        pv_config c = *cfg;
        c.effect = PV_PITCH_SHIFT;
        c.scale = ratios[k];
        pv_handle* h = nullptr;
        st = pv_create(&c, &h);
        if (st != PV_OK) {
            pv_harmonizer_destroy(hz);
            return st;
        }
        hz->voices.push_back(h);
    }
    *out = hz;
    return PV_OK;
}

pv_status pv_harmonizer_set_formant(pv_harmonizer* hz, int order) {
    if (!hz || hz->voices.empty()) return fail(PV_ERR_ARG, "null harmoniser");
    // voice 0 owns the envelope rows; a refusal leaves every voice as it was
    pv_status st = set_formant(hz->voices[0], order, true);
    if (st != PV_OK) return st;
    for (size_t k = 1; k < hz->voices.size(); ++k) (void)set_formant(hz->voices[k], order, false);
    return PV_OK;
}

pv_status pv_harmonize(pv_harmonizer* hz, const float* x, long long ldx, long long n_samples,
                       int channels, int frames, pv_float2* spec, long long ld_spec, float* voices_out,
                       long long ldo, long long ld_voice, const float* gains, float* mix,
                       long long ld_mix, void* stream) {
    if (!hz || hz->voices.empty()) return fail(PV_ERR_ARG, "null harmoniser");
    pv_handle* h0 = hz->voices[0];
    pv_status st = check_common(h0, channels, frames);
    if (st != PV_OK) return st;
    if (mix && !gains) return fail(PV_ERR_ARG, "mix needs gains");
    if (channels == 0 || frames == 0) return PV_OK;  // nothing to do (as pv_process)
    if (!voices_out) return fail(PV_ERR_ARG, "null voices_out");
    const int K = (int)hz->voices.size();
    const long long olen = pv_output_length(h0, frames);
    if (K > 1 && ld_voice < (long long)(channels - 1) * ldo + olen)
        return fail(PV_ERR_ARG, "ld_voice smaller than one voice's output block");
    DeviceGuard g(h0->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    st = do_analysis(h0, x, ldx, n_samples, channels, frames, spec, ld_spec, true, s);
    if (st != PV_OK) return st;
    st = do_resynthesis(h0, spec, ld_spec, channels, frames, nullptr, 0, voices_out, ldo, true, s,
                        nullptr, /*force_scan: other voices read h0's carries*/ true);
    if (st != PV_OK) return st;
    for (int k = 1; k < K; ++k) {
        // (formant preservation: voice 0 computed the envelope rows of the shared analysis)
        st = do_resynthesis(hz->voices[k], spec, ld_spec, channels, frames, nullptr, 0,
                            voices_out + (long long)k * ld_voice, ldo, true, s, h0->d_carry, false, nullptr,
                            hz->voices[k]->formant ? h0->d_env.p : nullptr);
        if (st != PV_OK) return st;
    }
    if (mix && channels > 0 && frames > 0) {
        if (K > 64) return fail(PV_ERR_ARG, "too many voices to mix");
        pv::MixParams mp{};
        mp.src = voices_out;
        mp.ldo = ldo;
        mp.ld_voice = ld_voice;
        mp.voices = K;
        for (int k = 0; k < K; ++k) mp.gain[k] = gains[k];
        mp.dst = mix;
        mp.ld_mix = ld_mix;
        mp.len = olen;
        mp.channels = channels;
        hipError_t e = pv::launch_mix(mp, s);
        if (e != hipSuccess) return fail(PV_ERR_HIP, std::string("mix launch: ") + hipGetErrorString(e));
    }
    return PV_OK;
}

}  // extern "C"
