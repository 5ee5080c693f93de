// dadd_latency -- the latency of a dependent fp64 add on this device: one wave runs a chain of
// N adds (each add's result is the next one's operand), timed with device events.  The lower
// bound of VCFX_inbreeding_calculator's per-sample chain is n_records x this figure
// (tools/ib_time.py).  Prints one JSON line.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

__global__ __launch_bounds__(64) void k_chain(double *out, double y, long n) {
    double x = (double)threadIdx.x;
    for (long i = 0; i < n; i += 16) {
#pragma unroll
        for (int u = 0; u < 16; u++) x = __dadd_rn(x, y);
    }
    out[threadIdx.x] = x;
}

int main() {
    const long n = 1L << 24;
    double *out = nullptr;
    if (hipMalloc(&out, 64 * sizeof(double)) != hipSuccess) {
        fprintf(stderr, "no device\n");
        return 1;
    }
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    std::vector<float> ms;
    for (int r = 0; r < 7; r++) {  // (the first two warm up)
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k_chain, dim3(1), dim3(64), 0, 0, out, 1.0e-9, n);
        (void)hipEventRecord(b, 0);
        if (hipEventSynchronize(b) != hipSuccess) return 1;
        float t = 0.f;
        (void)hipEventElapsedTime(&t, a, b);
        if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"adds\": %ld, \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"ns_per_dependent_add\": %.4f}\n", n,
           ms[ms.size() / 2], ms.front(), ms.back(), ms[ms.size() / 2] * 1e6 / (double)n);
    (void)hipFree(out);
    return 0;
}
