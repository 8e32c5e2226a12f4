// A derive text (MCX_DERIVE_SOURCE) of quantities that are no parameter: out[0] = the contrast x[0] - x[d-1] shifted by
// par[0], out[1] = |x[0] x[d-1]|, out[2] = log L itself; outputs past the third (when nout > 3) are the squares of the
// parameters in turn.  Only +, -, * and fabsf, each rounded to float, so that numpy float32 reproduces it bit for bit
// (tests/test_gpu_derive.py).  par = (shift).
__device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout)
{
  const float a = x[0], z = x[d - 1];
  out[0] = (a - z) + par[0];
  if (nout > 1) out[1] = fabsf(a * z);
  if (nout > 2) out[2] = ly;
  for (int j = 3; j < nout; ++j) out[j] = x[j % d] * x[j % d];
}
