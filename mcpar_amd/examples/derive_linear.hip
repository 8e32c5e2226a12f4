// A derive text (MCX_DERIVE_SOURCE) that restates MCX_DERIVE_LINEAR: par = A[nout][d] row-major, then b[nout], and
// out[j] = b[j] + A[j][0] x[0] + ... + A[j][d-1] x[d-1] added in that order, every product and every sum rounded to float
// (the text is compiled with -ffp-contract=off: no fma).  Same bytes as the built-in for the same A and b
// (tests/test_gpu_derive.py); the place to start from for a map the built-in does not cover.
__device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout)
{
  for (int j = 0; j < nout; ++j) {
    float acc = par[nout * d + j];
    for (int k = 0; k < d; ++k) acc = acc + par[j * d + k] * x[k];
    out[j] = acc;
  }
}
