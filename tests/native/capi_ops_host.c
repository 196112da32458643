/* capi_ops_host.c -- the INTEGRATION.md "operand block" example as a program: build a --scale kernel (a heterogeneous heat step,
 * u' = u + w * L(u)) through the C ABI, run the ping-pong loop through drs_kernel_run_ops on device buffers, run the gold kernel on a
 * second pair with the same operands, compare with checkError3D semantics; then the refusals: an old entry point on a --scale kernel,
 * a missing operand, a superfluous one, a wrong size.  usage: capi_ops_host <3d .stc> <L> <M> <N> <halo> */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include "drstencil_amd.h"

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int L = atoi(argv[2]), M = atoi(argv[3]), N = atoi(argv[4]), H = atoi(argv[5]);
    const size_t n = (size_t)L * M * N, nbytes = n * sizeof(float);
    const char *args[] = {"--3d", "--dtype", "fp32", "--scale", "--scale-centre", "1", argv[1]};
    char *log = NULL;
    drs_kernel *k = drs_kernel_build(7, args, NULL, &log);          /* runs hipcc on a cache miss: before any HIP call */
    if (!k) { printf("build failed: %s\n", log ? log : ""); return 1; }
    float *h = (float *)malloc(nbytes), *hw = (float *)malloc(nbytes), *out = (float *)malloc(nbytes), *ref = (float *)malloc(nbytes);
    drs_fill_random_f32(h, n, 1);
    drs_fill_random_f32(hw, n, 2);
    for (size_t x = 0; x < n; x++) hw[x] = 0.5f + 0.5f * hw[x];     /* kappa dt / h^2 in [0.5, 1) */
    void *a, *b, *ga, *gb, *w;
    if (hipMalloc(&a, nbytes) || hipMalloc(&b, nbytes) || hipMalloc(&ga, nbytes) || hipMalloc(&gb, nbytes) || hipMalloc(&w, nbytes)) { printf("hipMalloc failed\n"); return 1; }
    hipMemcpy(a, h, nbytes, hipMemcpyHostToDevice); hipMemset(b, 0, nbytes);
    hipMemcpy(ga, h, nbytes, hipMemcpyHostToDevice); hipMemset(gb, 0, nbytes);
    hipMemcpy(w, hw, nbytes, hipMemcpyHostToDevice);
    drs_operands ops = {sizeof(drs_operands), NULL, NULL, NULL, w};
    float ms = 0.f;
    int launches = drs_kernel_run_timed_ops(k, a, b, &ops, 4, 0, NULL, &ms);      /* no warm-up: the result must equal one gold run */
    int glaunches = drs_kernel_run_ops(k, ga, gb, &ops, 4, 1, NULL);
    int one = drs_kernel_launch_ops(k, a, b, &ops, NULL), gone = drs_kernel_launch_gold_ops(k, ga, gb, &ops, NULL);
    hipDeviceSynchronize();
    hipMemcpy(out, b, nbytes, hipMemcpyDeviceToHost);
    hipMemcpy(ref, gb, nbytes, hipMemcpyDeviceToHost);
    double max_abs, max_rel; long at;
    double rms = drs_check_error_f32(3, L, M, N, H, out, ref, &max_abs, &at, &max_rel);
    printf("launches %d gold_launches %d one %d gold_one %d ms_positive %d rms %.3e max_abs %.3e max_rel %.3e\n", launches, glaunches, one, gone, ms > 0.f, rms, max_abs, max_rel);
    drs_operands none = {sizeof(drs_operands), NULL, NULL, NULL, NULL}, extra = {sizeof(drs_operands), w, NULL, NULL, w}, small = {sizeof(drs_operands) - 8, NULL, NULL, NULL, w};
    printf("refusals old %d missing %d superfluous %d size %d solve %d\n", drs_kernel_launch(k, a, b, NULL), drs_kernel_launch_ops(k, a, b, &none, NULL),
           drs_kernel_launch_ops(k, a, b, &extra, NULL), drs_kernel_launch_ops(k, a, b, &small, NULL), drs_kernel_solve_ops(k, a, b, &ops, 1e-3, 8, 1, NULL, NULL, NULL));
    drs_kernel_close(k);
    return 0;
}
