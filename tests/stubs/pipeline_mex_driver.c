/* TEST INFRASTRUCTURE: calls matlab/landing_pipeline_mex.c's mexFunction on arrays handed over by ctypes (tests/test_pipeline_cpu.py,
 * tests/test_gpu_pipeline.py). */
#include "mex.h"
char g_mex_err[512];
jmp_buf g_mex_jmp;
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);
const char* gateway_error(void) { return g_mex_err; }
/* data[i]: column-major buffer of argument i of n_args (21, or fewer to provoke the count check); ndim[i], dims[4*i..]: its MATLAB dimensions;
 * cls[i]: 6 double, 7 single.  n_opt (name, value) scalar pairs form the options struct; n_opt < 0 = none.  nlhs outputs are requested; X, F,
 * status, iters, kkt are [B] columns, pin / pout [kept] columns (*kept receives the column count of PAIR_IN).  Returns 0, or 1 after mexErrMsgTxt. */
int call_pipeline_gateway(int n_args, const double* const* data, const int* ndim, const int* dims, const int* cls, int n_opt, const char* const* opt_name,
                          const double* opt_val, int nlhs, double* X, double* F, int* status, int* iters, double* kkt, double* pin, double* pout, int nxk, int B,
                          int* kept) {
  mxArray* in[22]; mxArray* out[7] = {0, 0, 0, 0, 0, 0, 0}; int i, j, nrhs = n_args;
  g_mex_err[0] = 0;
  for (i = 0; i < n_args; ++i) {
    mwSize d[4]; size_t n = 1;
    for (j = 0; j < ndim[i]; ++j) { d[j] = (mwSize)dims[4 * i + j]; n *= d[j]; }
    in[i] = mx_new((mwSize)ndim[i], d, (mxClassID)cls[i]);
    if (cls[i] == mxDOUBLE_CLASS) memcpy(in[i]->data, data[i], n * sizeof(double));
  }
  if (n_opt >= 0) {
    mwSize one[2] = {1, 1};
    mxArray* s = mx_new(2, one, mxSTRUCT_CLASS);
    for (i = 0; i < n_opt; ++i) { s->fname[s->nfields] = opt_name[i]; s->fval[s->nfields] = mxCreateDoubleMatrix(1, 1, mxREAL); *mxGetPr(s->fval[s->nfields]) = opt_val[i]; s->nfields++; }
    in[n_args] = s; nrhs = n_args + 1;
  }
  if (setjmp(g_mex_jmp)) return 1;
  mexFunction(nlhs, out, nrhs, (const mxArray**)in);
  if (X && out[0]) memcpy(X, out[0]->data, sizeof(double) * (size_t)nxk * B);
  if (F && out[1]) memcpy(F, out[1]->data, sizeof(double) * B);
  if (status && out[2]) memcpy(status, out[2]->data, sizeof(int) * 3 * B);
  if (iters && out[3]) memcpy(iters, out[3]->data, sizeof(int) * 3 * B);
  if (kkt && out[4]) memcpy(kkt, out[4]->data, sizeof(double) * 3 * B);
  *kept = out[5] ? (int)out[5]->dims[1] : -1;
  if (pin && out[5]) memcpy(pin, out[5]->data, sizeof(double) * 9 * out[5]->dims[1]);
  if (pout && out[6]) memcpy(pout, out[6]->data, sizeof(double) * (size_t)nxk * out[6]->dims[1]);
  for (i = 1; i < 7; ++i) if (i >= (nlhs > 1 ? nlhs : 1) && out[i]) return 2;      /* an output nobody asked for was created */
  return 0;
}
