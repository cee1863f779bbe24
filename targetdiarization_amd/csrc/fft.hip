// fft.hip — the C-ABI of the any-length FFT and of the band mix (include/tdx.h).  The kernels, the planner and the
// drivers are in fft.hpp; here are the argument rules.  Nothing is allocated and no state is kept: the entry points issue kernel
// launches on the caller's stream and nothing else.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/tdx.h"
#include "fft.hpp"

using namespace tdx;

namespace {

constexpr int tile_log2_of(int t) { return t <= 1 ? 0 : 1 + tile_log2_of(t / 2); }
constexpr int TILE_LOG2 = tile_log2_of(TDX_FFT_TILE);
static_assert((1 << TILE_LOG2) == TDX_FFT_TILE && TILE_LOG2 >= fft::MIN_TILE_LOG2 && TILE_LOG2 <= fft::MAX_TILE_LOG2, "TDX_FFT_TILE: a power of two in 2^4 .. 2^12");

inline size_t ws_floats(long n, int batch) {
    return std::max(fft::c2c_ws_floats(n, batch, TILE_LOG2), std::max(fft::r2c_ws_floats(n, batch, TILE_LOG2), fft::c2r_ws_floats(n, batch, TILE_LOG2)));
}
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// the checks every transform shares; `what` names the two data pointers in the messages
int check_common(const char* fn, const void* in, const void* out, long n, int batch, const void* ws, size_t ws_bytes) {
    const std::string f(fn);
    if (!in || !out || !ws) return tdx::fail(TDX_E_INVALID, f + ": null argument");
    if (n < 1 || n > fft::MAX_N) return tdx::fail(TDX_E_INVALID, f + ": need 1 <= n <= 2^26");
    if (batch < 1 || batch > fft::MAX_BATCH) return tdx::fail(TDX_E_INVALID, f + ": need 1 <= batch <= 65535");
    if (in == out) return tdx::fail(TDX_E_INVALID, f + ": in-place operation is not supported (input and output must not overlap)");
    if (!aligned8(in) || !aligned8(out) || !aligned8(ws)) return tdx::fail(TDX_E_INVALID, f + ": pointers must be 8-byte aligned (the kernels read and write pairs of floats, real "
                                                                                              "rows of even length included)");
    if (ws_bytes < tdx_fft_workspace_bytes(n, batch)) return tdx::fail(TDX_E_INVALID, f + ": workspace smaller than tdx_fft_workspace_bytes(n, batch)");
    return TDX_OK;
}

}  // namespace

extern "C" {

size_t tdx_fft_workspace_bytes(long n, int batch) {
    if (fft::size_error(n, batch)) return 0;
    return std::max<size_t>(ws_floats(n, batch), 64) * sizeof(float);
}

int tdx_fft_c2c(const float* x_dev, long n, int batch, int inverse, float* y_dev, void* ws, size_t ws_bytes, void* stream) {
    TRY(check_common("tdx_fft_c2c", x_dev, y_dev, n, batch, ws, ws_bytes));
    return fft::c2c(x_dev, n, batch, inverse != 0, y_dev, (float*)ws, TILE_LOG2, (hipStream_t)stream);
}

int tdx_fft_r2c(const float* x_dev, long n, int batch, float* X_dev, void* ws, size_t ws_bytes, void* stream) {
    TRY(check_common("tdx_fft_r2c", x_dev, X_dev, n, batch, ws, ws_bytes));
    return fft::r2c(x_dev, n, batch, X_dev, (float*)ws, TILE_LOG2, (hipStream_t)stream);
}

int tdx_fft_c2r(const float* X_dev, long n, int batch, float* y_dev, void* ws, size_t ws_bytes, void* stream) {
    TRY(check_common("tdx_fft_c2r", X_dev, y_dev, n, batch, ws, ws_bytes));
    return fft::c2r(X_dev, n, batch, y_dev, (float*)ws, TILE_LOG2, (hipStream_t)stream);
}

size_t tdx_fft_band_mix_workspace_bytes(long n) {
    if (n < 2 || n > fft::MAX_N) return 0;
    return fft::mix_ws(n, TILE_LOG2).total * sizeof(float);
}

int tdx_fft_band_mix(const float* main_dev, const float* aux_dev, long n, const long ranges[6], float* y_dev, float* tap_main, float* tap_aux,
                     float* tap_mix, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "tdx_fft_band_mix: ";
    if (!main_dev || !aux_dev || !ranges || !y_dev || !ws) return tdx::fail(TDX_E_INVALID, std::string(fn) + "null argument");
    if (n < 2 || n > fft::MAX_N) return tdx::fail(TDX_E_INVALID, std::string(fn) + "need 2 <= n <= 2^26");
    static const char* const names[3] = {"main", "aux", "overlap"};
    fft::MixRanges rg;
    for (int i = 0; i < 3; ++i) {
        rg.lo[i] = ranges[2 * i]; rg.hi[i] = ranges[2 * i + 1];
        if (rg.lo[i] < 0 || rg.lo[i] > rg.hi[i] || rg.hi[i] > n / 2 + 1)
            return tdx::fail(TDX_E_INVALID, std::string(fn) + "the " + names[i] + " bin range must satisfy 0 <= lo <= hi <= n / 2 + 1");
    }
    if (y_dev == main_dev || y_dev == aux_dev) return tdx::fail(TDX_E_INVALID, std::string(fn) + "in-place operation is not supported (input and output must not overlap)");
    if (!aligned8(y_dev) || !aligned8(ws) || !aligned8(tap_main) || !aligned8(tap_aux) || !aligned8(tap_mix))
        return tdx::fail(TDX_E_INVALID, std::string(fn) + "y_dev, the taps and the workspace must be 8-byte aligned (the kernels write pairs of floats)");
    if (ws_bytes < tdx_fft_band_mix_workspace_bytes(n)) return tdx::fail(TDX_E_INVALID, std::string(fn) + "workspace smaller than tdx_fft_band_mix_workspace_bytes(n)");
    return fft::band_mix(main_dev, aux_dev, n, rg, y_dev, tap_main, tap_aux, tap_mix, (float*)ws, TILE_LOG2, (hipStream_t)stream);
}

}  // extern "C"
