/* The correctly rounded fused multiply-add of libm over arrays: the arithmetic of the --varcoef host reference (tests/varcoef_cases.py).
 * TEST INFRASTRUCTURE.  Compiled without -mfma and with -ffp-contract=off, so every element is one call of fmaf / fma. */
#include <math.h>
#include <stddef.h>

void vc_fmaf(const float *a, const float *b, const float *c, float *out, size_t n)
{
    for (size_t i = 0; i < n; i++) out[i] = fmaf(a[i], b[i], c[i]);
}

void vc_fma(const double *a, const double *b, const double *c, double *out, size_t n)
{
    for (size_t i = 0; i < n; i++) out[i] = fma(a[i], b[i], c[i]);
}
