// gfx950 fp64 matrix-core rate: back-to-back v_mfma_f64_16x16x4_f64 (__builtin_amdgcn_mfma_f64_16x16x4f64) on A independent
// accumulators per wave, no memory traffic in the loop.  Launches: one workgroup of 4 waves (one wave per SIMD of one CU), one such
// workgroup per CU, and two per CU (two waves per SIMD); the best of 5 runs each.  Prints cycles per instruction and SIMD (wall time
// at the nominal 2.4 GHz) and the chip's rate in TFLOP/s (2 * 16 * 16 * 4 per instruction).
// build: hipcc --offload-arch=gfx950 -O3 -o mfma_f64_rate mfma_f64_rate.hip (tools/mb_mfma.sh builds and runs it)
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef double v4d __attribute__((ext_vector_type(4)));

template <int A>
__global__ __launch_bounds__(256) void k_mfma(double *out, int iters)
{
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    v4d acc[A];
#pragma unroll
    for (int j = 0; j < A; j++) acc[j] = v4d{0.0, 0.0, 0.0, (double)j};
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int r = 0; r < 16 / A; r++)
#pragma unroll
            for (int j = 0; j < A; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
    }
    double s = 0;
#pragma unroll
    for (int j = 0; j < A; j++) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int A>
static void run(int n_cu, int blocks, int threads, int iters, const char *what)
{
    double *d;
    hipMalloc(&d, (size_t)blocks * threads * sizeof(double));
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    k_mfma<A><<<blocks, threads>>>(d, 8);                       // warm-up
    hipDeviceSynchronize();
    float best = 1e30f;
    for (int rep = 0; rep < 5; rep++) {
        hipEventRecord(e0);
        k_mfma<A><<<blocks, threads>>>(d, iters);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    const double waves = (double)blocks * threads / 64, inst = waves * iters * 16;
    const double simds = blocks >= n_cu ? 4.0 * n_cu : 4.0 * blocks;          // SIMDs that hold a wave
    const double per_simd = inst / simds;
    const double cyc = best * 1e-3 * 2.4e9 / per_simd;
    printf("%-34s acc %d: %8.3f ms  %.3e inst  %6.2f cycles / inst / SIMD @2.4 GHz  %7.2f TFLOP/s\n", what, A, best, inst, cyc,
           inst * 2048.0 / (best * 1e-3) / 1e12);
    hipFree(d);
}

int main()
{
    hipDeviceProp_t p;
    hipGetDeviceProperties(&p, 0);
    const int n_cu = p.multiProcessorCount;
    printf("%s, %d CUs, clock %d kHz\n", p.gcnArchName, n_cu, p.clockRate);
    run<1>(n_cu, 1, 256, 20000, "one CU, one wave per SIMD");
    run<2>(n_cu, 1, 256, 20000, "one CU, one wave per SIMD");
    run<4>(n_cu, 1, 256, 20000, "one CU, one wave per SIMD");
    run<8>(n_cu, 1, 256, 20000, "one CU, one wave per SIMD");
    run<1>(n_cu, n_cu, 256, 20000, "every CU, one wave per SIMD");
    run<4>(n_cu, n_cu, 256, 20000, "every CU, one wave per SIMD");
    run<8>(n_cu, n_cu, 256, 20000, "every CU, one wave per SIMD");
    run<4>(n_cu, 2 * n_cu, 256, 20000, "every CU, two waves per SIMD");
    return 0;
}
