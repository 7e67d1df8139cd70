// What one scalar v_fma_f32 costs against one v_pk_fma_f32 (two f32 lanes per instruction) on gfx950, at 1..8 waves per SIMD.
// valu_rate.hip cannot tell: its fmaf() chains are re-packed by the compiler's SLP vectoriser.  Here every instruction is an
// `asm volatile` statement of its own, 8 independent chains per lane, so what is timed is what is written.  Beside the two
// f32 forms: v_fma_f64 (the yardstick), v_mov_b64, v_max_f64 and v_cmp_gt_f64 - the instructions the solver's convergence
// test and iterate copies are made of (csrc/lfd_geometry.hpp).
//   hipcc --offload-arch=gfx950 -O3 profiles/microbench/fma_f32_packing.hip -o profiles/microbench/fma_f32_packing
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kIters = 4096;
constexpr int kChains = 8;
typedef float v2f __attribute__((ext_vector_type(2)));

template <int OP>
__global__ void __launch_bounds__(256) chain_kernel(double* out, float seed, int iters) {
    float f[kChains];
    v2f p[kChains];
    double d[kChains], e[kChains];
    for (int i = 0; i < kChains; ++i) {
        f[i] = seed + i + threadIdx.x;
        p[i] = v2f{f[i], f[i] + 0.5f};
        d[i] = (double)f[i];
        e[i] = d[i] + 1.0;
    }
    const float fm = seed * 0.999f, fc = seed * 0.5f;
    const v2f pm = {fm, fm}, pc = {fc, fc};
    const double dm = (double)fm, dc = (double)fc;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < kChains; ++i) {
            if (OP == 0) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[i]) : "v"(fm), "v"(fc));
            if (OP == 1) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "v"(pm), "v"(pc));
            if (OP == 2) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(f[i]) : "v"(fm));
            if (OP == 3) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p[i]) : "v"(pm));
            if (OP == 4) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[i]) : "v"(dm), "v"(dc));
            if (OP == 5) asm volatile("v_mov_b64 %0, %1" : "=v"(e[i]) : "v"(d[i]));
            if (OP == 6) asm volatile("v_max_f64 %0, %0, %1" : "+v"(d[i]) : "v"(dm));
            if (OP == 7) asm volatile("v_cmp_gt_f64 vcc, %0, %1" :: "v"(d[i]), "v"(dm) : "vcc");
        }
    }
    double s = 0.0;
    for (int i = 0; i < kChains; ++i) s += (double)f[i] + (double)p[i].x + (double)p[i].y + d[i] + e[i];
    if (s == 1.2345e-300) out[0] = s;
}

template <int OP>
double run(const char* name, int waves_per_simd) {
    hipDeviceProp_t p; CHK(hipGetDeviceProperties(&p, 0));
    const int blocks = p.multiProcessorCount * waves_per_simd;     // 256 threads = 4 waves = one per SIMD
    double* d; CHK(hipMalloc(&d, 8));
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    chain_kernel<OP><<<blocks, 256>>>(d, 1.000001f, 16);
    CHK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
        CHK(hipEventRecord(e0));
        chain_kernel<OP><<<blocks, 256>>>(d, 1.000001f, kIters);
        CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
        float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double insts = (double)kIters * kChains * waves_per_simd;
    const double clk = (double)p.clockRate * 1e3;
    const double cyc = best * 1e-3 * clk / insts;
    printf("%-14s waves/SIMD %d  %.3f ms  %.2f cycles per wave-instruction (at %.0f MHz nominal)\n", name, waves_per_simd, best, cyc, clk / 1e6);
    CHK(hipEventDestroy(e0)); CHK(hipEventDestroy(e1)); CHK(hipFree(d));
    return cyc;
}

int main() {
    for (int w : {1, 2, 4, 8}) {
        const double s = run<0>("v_fma_f32", w);
        const double k = run<1>("v_pk_fma_f32", w);
        run<2>("v_mul_f32", w);
        run<3>("v_pk_mul_f32", w);
        run<4>("v_fma_f64", w);
        run<5>("v_mov_b64", w);
        run<6>("v_max_f64", w);
        run<7>("v_cmp_gt_f64", w);
        printf("  waves/SIMD %d: one v_pk_fma_f32 costs %.2f scalar v_fma_f32 (two scalar ones do the same work: packed is %s)\n", w, k / s,
               k < 2.0 * s ? "cheaper per f32 operation" : "no cheaper per f32 operation");
    }
    return 0;
}
