/* TEST INFRASTRUCTURE: a hand-written stand-in for an emitted plugin (same three entry points), used only by the self-test of the
 * memory-footprint harness (tests/test_memory_footprint_cpu.py) and only on the CPU.  It computes the 2D 5-point star of the
 * self-test's spec in fp64 in the oracle's contracted order (t = c0*a0; t = fma(ci, ai, t), taps sorted by (j, i)) and, when the
 * environment variable FOOTPRINT_DEFECT names one, commits that memory-contract violation in drs_plugin_launch (the gold entry point
 * stays clean):
 *   read_past_end       loads the element right behind the input array
 *   write_before_start  stores to the element right before the output array
 *   nan_leak            lets the input's corner cell (which no tap reads) reach an output through 0 * x
 *   ring_write          stores to a ring cell of the output
 * Compile with -DFP_M=<rows> -DFP_N=<columns> -ffp-contract=off. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define STR_(x) #x
#define STR(x) STR_(x)

static const int TJ[5] = {-1, 0, 0, 0, 1};
static const int TI[5] = {0, -1, 0, 1, 0};
static const double TC[5] = {0.2, 0.25, 0.3, 0.15, 0.1};

static void sweep(const double *in, double *out)
{
    for (int j = 1; j < FP_M - 1; j++)
        for (int i = 1; i < FP_N - 1; i++) {
            double t = TC[0] * in[(j + TJ[0]) * FP_N + i + TI[0]];
            for (int p = 1; p < 5; p++)
                t = fma(TC[p], in[(j + TJ[p]) * FP_N + i + TI[p]], t);
            out[j * FP_N + i] = t;
        }
}

int drs_plugin_launch_gold(const void *in, void *out, void *stream)
{
    (void)stream;
    sweep((const double *)in, (double *)out);
    return 0;
}

int drs_plugin_launch(const void *in_, void *out_, void *stream)
{
    const volatile double *in = (const volatile double *)in_;
    volatile double *out = (volatile double *)out_;
    const char *d = getenv("FOOTPRINT_DEFECT");
    (void)stream;
    sweep((const double *)in_, (double *)out_);
    if (!d || !*d)
        return 0;
    if (!strcmp(d, "read_past_end")) {
        volatile double sink = in[FP_M * FP_N];
        (void)sink;
    } else if (!strcmp(d, "write_before_start")) {
        out[-1] = 0.0;
    } else if (!strcmp(d, "nan_leak")) {
        out[1 * FP_N + 1] = out[1 * FP_N + 1] + 0.0 * in[0];
    } else if (!strcmp(d, "ring_write")) {
        out[FP_N / 2] = 1.0;
    } else {
        return 1;
    }
    return 0;
}

const char *drs_plugin_info(void)
{
    return "{\"name\":\"footprint_selftest\",\"ndim\":2,\"M\":" STR(FP_M) ",\"N\":" STR(FP_N) ",\"halo\":1,\"step\":1,\"stages\":1}";
}
