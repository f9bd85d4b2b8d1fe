// fluidlab_amd/csrc/fe_smoke_index.h as the host and the GPU compile it: sm_tri_axis, the one-axis back-trace index of the smoke solver, one
// case per lane.  The header is included unchanged.  Built twice by tests/smoke_index_cases.py:
//   host library    --offload-host-only -DSIT_HOST_ONLY: sit_axis_host alone (tests/test_smoke_index.py, no GPU);
//   device library  hipcc + the engine's flags: sit_axis runs the kernel (host pointers in and out; the return value is the first HIP error)
//                   and sit_axis_host the same function on the CPU (tests/test_smoke_index_hip.py).
// The kernel only computes: what it writes is indexed by the lane's own number, never by what it computed.
#include <cstddef>
#include <cmath>
#include <hip/hip_runtime.h>
#include "../../fluidlab_amd/csrc/fe_smoke_index.h"

__host__ __device__ inline void sit_one(const float* p, int n, int* base, float* f, int* c0, int* c1, int i) {
    sm_tri_axis(p[i], n, base[i], f[i], c0[i], c1[i]);
}

extern "C" int sit_axis_host(const float* p, int n, int* base, float* f, int* c0, int* c1, int count) {
    for (int i = 0; i < count; i++) sit_one(p, n, base, f, c0, c1, i);
    return 0;
}

#ifndef SIT_HOST_ONLY
__global__ __launch_bounds__(256) void k_sit_axis(const float* p, int n, int* base, float* f, int* c0, int* c1, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    sit_one(p, n, base, f, c0, c1, i);
}

// Every buffer is sized from count; the first HIP error is kept, nothing is launched or copied after it, everything is freed.
extern "C" int sit_axis(const float* p, int n, int* base, float* f, int* c0, int* c1, int count) {
    if (count <= 0) return 0;
    const size_t bytes = 4 * (size_t)count;                      // (float and int are four bytes each)
    void* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    void* h[5] = {(void*)p, base, f, c0, c1};
    hipError_t err = hipSuccess;
    auto note = [&](hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; };
    for (int k = 0; k < 5 && err == hipSuccess; k++) note(hipMalloc(&d[k], bytes));
    if (err == hipSuccess) note(hipMemcpy(d[0], p, bytes, hipMemcpyHostToDevice));
    for (int k = 1; k < 5 && err == hipSuccess; k++) note(hipMemset(d[k], 0xFF, bytes));     // a word no lane wrote reads as NaN / -1
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_sit_axis, dim3((unsigned)(((size_t)count + 255) / 256)), dim3(256), 0, 0, (const float*)d[0], n, (int*)d[1], (float*)d[2],
                           (int*)d[3], (int*)d[4], count);
        note(hipGetLastError()); note(hipDeviceSynchronize());
    }
    for (int k = 1; k < 5 && err == hipSuccess; k++) note(hipMemcpy(h[k], d[k], bytes, hipMemcpyDeviceToHost));
    for (int k = 0; k < 5; k++) if (d[k]) note(hipFree(d[k]));
    return (int)err;
}
#endif
