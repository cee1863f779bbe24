// weight_planes.hpp — the weights of the split-f16 x3 core (gemm_h3.hpp), made once at create: every [N][K] fp32 matrix of
// a model as f16 planes [N][K] x 4 bytes followed by its al(N) row scales, all in one allocation.
#pragma once
#include <vector>

#include "gemm_h3.hpp"
#include "tdx_common.hpp"

namespace tdx {

struct PlaneJob {
    const float* w; long N, K;                      // device matrix [N][K], K contiguous
    const unsigned char** planes; const float** scales;      // where the pointers into the allocation go
    // launch_h3_split_rows_long for rows beyond 2048 floats.  (A pointer, not a flag: the split kernels are templates, and a
    // branch to the long one here would instantiate it in every translation unit that splits weights.)
    hipError_t (*split)(const float*, long, void*, float*, long, int, hipStream_t) = launch_h3_split_rows;
};

// allocates `planes` on `device`, splits the jobs in order on its null stream and waits for them
inline int split_weight_planes(const std::vector<PlaneJob>& jobs, int device, DevBuf& planes) {
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, __FILE__, __LINE__);
    size_t bytes = 0;
    for (const PlaneJob& j : jobs) bytes += (size_t)j.N * j.K * 4 + al(j.N) * 4;
    hipError_t e = planes.alloc(bytes);
    if (e != hipSuccess) return fail_hip(e, __FILE__, __LINE__);
    unsigned char* q = static_cast<unsigned char*>(planes.get());
    for (const PlaneJob& j : jobs) {
        float* sc = (float*)(q + (size_t)j.N * j.K * 4);
        e = j.split(j.w, j.K, q, sc, j.N, (int)j.K, nullptr);
        if (e != hipSuccess) return fail_hip(e, __FILE__, __LINE__);
        *j.planes = q; *j.scales = sc;
        q += (size_t)j.N * j.K * 4 + al(j.N) * 4;
    }
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail_hip(e, __FILE__, __LINE__);
    return 0;
}

}  // namespace tdx
