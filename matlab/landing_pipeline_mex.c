/* landing_pipeline_mex.c -- MATLAB gateway of the drop-state chain (mex -> C ABI -> HIP): what generate_data/generate_training_data_automated.m:130-219
 * does per sample -- the SRBM solve, the kinodynamic (KNITRO) solve from [X*; jpos_guess; U*], the `_ws` re-solve from that solution, the training pair --
 * for B drop states in one call:
 *   [X, F, STATUS, ITERS, KKT, PAIR_IN, PAIR_OUT] = landing_pipeline_mex(Xref, Uref, dt, ..., Ib_inv [, opts])
 * The 21 arguments of landing_solve_mex.c in the same order and with the same rules (B = third dimension of Xref; every other argument holds B members
 * or ONE member shared by the batch).  Outputs (created only when asked for):
 *   X (48N+12) x B     the final kinodynamic solution [X(:); jpos(:); U(:)] (the re-solve's if it converged, else the first solve's if that converged)
 *   F 1 x B, KKT 3 x B, STATUS / ITERS int32 3 x B (rows: SRBM solve, kinodynamic solve, re-solve; STATUS as in landing_refine_mex.c)
 *   PAIR_IN 9 x M, PAIR_OUT (48N+12) x M   the training columns [rpy0; omega0; v0] -> [X*(:); U*(:); jpos*(:)] of the M members that converged (:204-219)
 * opts (optional struct): device (HIP device index, default 0), warm (0: no re-solve; default 1), kin_box_x0 / kin_box_y0 (default 0.125 / 0.125, the
 * literals of generate_landingCtrller_KNITRO.m), max_iter_srbm / max_iter_refine / max_iter_resolve, tol (all three passes).
 * Build:  mex landing_pipeline_mex.c -I<repo>/include -L<repo>/landing-controller_amd -llanding_mi355x
 * The chain itself lives in landing_pipeline_21_on (include/landing_nlp.h). */
#include <string.h>
#include "mex.h"
#include "landing_nlp.h"

static double opt_scalar(const mxArray* o, const char* name, double dflt) {
  const mxArray* f = o ? mxGetField(o, 0, name) : NULL;
  if (!f || mxIsEmpty(f)) return dflt;
  if (!mxIsDouble(f) && !mxIsLogical(f)) mexErrMsgTxt("landing_pipeline_mex: option fields must be double or logical scalars");
  return mxGetScalar(f);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  static const char* names[21] = {"Xref", "Uref", "dt", "q_min", "q_max", "qd_min", "qd_max", "q_init", "qd_init", "q_term_min", "q_term_max",
                                  "qd_term_min", "qd_term_max", "QN", "x0", "mu", "l_leg_max", "f_max", "mass", "Ib", "Ib_inv"};
  const double* a[21]; double* tmp[21]; size_t per[21]; int i, b, N, B, device, kept = 0, rc;
  long long nxk, ngk;
  char msg[256];
  landing_pipeline_opts o;
  const mxArray* os = nrhs == 22 ? prhs[21] : NULL;
  double *X, *F, *KK, *pin, *pout;
  int *st, *it;
  if (nrhs != 21 && nrhs != 22) mexErrMsgTxt("landing_pipeline_mex: 21 inputs (generate_landingCtrller_IPOPT.m:323-327) and an optional options struct");
  if (nlhs > 7) mexErrMsgTxt("landing_pipeline_mex: at most 7 outputs [X, F, STATUS, ITERS, KKT, PAIR_IN, PAIR_OUT]");
  for (i = 0; i < 21; ++i) if (!mxIsDouble(prhs[i]) || mxIsComplex(prhs[i]) || mxIsSparse(prhs[i])) {
    snprintf(msg, sizeof(msg), "landing_pipeline_mex: argument %d (%s) must be a full real double array", i + 1, names[i]); mexErrMsgTxt(msg); }
  {
    const mwSize* d = mxGetDimensions(prhs[0]); const mwSize nd = mxGetNumberOfDimensions(prhs[0]);
    if (nd < 2 || nd > 3 || d[0] != 12 || d[1] < 3) mexErrMsgTxt("landing_pipeline_mex: Xref must be 12 x (N+1) [x B]");
    N = (int)d[1] - 1; B = nd > 2 ? (int)d[2] : 1;
  }
  if (B < 1 || landing_kinodyn_nlp_dims(N, &nxk, &ngk)) mexErrMsgTxt("landing_pipeline_mex: empty batch or unsupported horizon (2 <= N <= 64 intervals)");
  for (i = 0; i < 21; ++i) per[i] = 6;
  per[0] = 12 * (size_t)(N + 1); per[1] = 24 * (size_t)N; per[2] = (size_t)N; per[13] = 12; per[14] = (size_t)landing_nx(N);
  per[15] = per[16] = per[17] = per[18] = 1; per[19] = per[20] = 3;
  for (i = 0; i < 21; ++i) tmp[i] = NULL;
  for (i = 0; i < 21; ++i) {
    const size_t n = mxGetNumberOfElements(prhs[i]);
    if (n == per[i] * (size_t)B) a[i] = mxGetPr(prhs[i]);
    else if (n == per[i]) {        /* one member's worth: shared by the batch */
      tmp[i] = (double*)mxMalloc(per[i] * (size_t)B * sizeof(double));
      for (b = 0; b < B; ++b) memcpy(tmp[i] + (size_t)b * per[i], mxGetPr(prhs[i]), per[i] * sizeof(double));
      a[i] = tmp[i];
    } else {
      snprintf(msg, sizeof(msg), "landing_pipeline_mex: argument %d (%s) has %lu elements; expected %lu (one member) or %lu (B = %d members, N = %d)",
               i + 1, names[i], (unsigned long)n, (unsigned long)per[i], (unsigned long)(per[i] * (size_t)B), B, N);
      for (b = 0; b < i; ++b) if (tmp[b]) mxFree(tmp[b]);
      mexErrMsgTxt(msg);
    }
  }
  if (os && !mxIsEmpty(os) && !mxIsStruct(os)) mexErrMsgTxt("landing_pipeline_mex: the 22nd argument must be an options struct");
  if (os && mxIsEmpty(os)) os = NULL;
  landing_pipeline_opts_default(&o);
  device = (int)opt_scalar(os, "device", 0.0);
  o.warm = opt_scalar(os, "warm", 1.0) != 0.0;
  o.form.kin_box_x0 = opt_scalar(os, "kin_box_x0", o.form.kin_box_x0); o.form.kin_box_y0 = opt_scalar(os, "kin_box_y0", o.form.kin_box_y0);
  o.srbm.max_iter = (int)opt_scalar(os, "max_iter_srbm", (double)o.srbm.max_iter);
  o.refine.max_iter = (int)opt_scalar(os, "max_iter_refine", (double)o.refine.max_iter);
  o.resolve.max_iter = (int)opt_scalar(os, "max_iter_resolve", (double)o.resolve.max_iter);
  o.srbm.tol = o.refine.tol = o.resolve.tol = opt_scalar(os, "tol", o.srbm.tol);
  X = (double*)mxMalloc((size_t)nxk * B * sizeof(double)); F = (double*)mxMalloc((size_t)B * sizeof(double)); KK = (double*)mxMalloc(3 * (size_t)B * sizeof(double));
  pin = (double*)mxMalloc(9 * (size_t)B * sizeof(double)); pout = (double*)mxMalloc((size_t)nxk * B * sizeof(double));
  st = (int*)mxMalloc(3 * (size_t)B * sizeof(int)); it = (int*)mxMalloc(3 * (size_t)B * sizeof(int));
  rc = landing_pipeline_21_on(device, N, B, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], a[16], a[17],
                              a[18], a[19], a[20], &o, X, F, NULL, st, it, KK, pin, pout, &kept);
  for (i = 0; i < 21; ++i) if (tmp[i]) mxFree(tmp[i]);
  if (rc) {
    mxFree(X); mxFree(F); mxFree(KK); mxFree(pin); mxFree(pout); mxFree(st); mxFree(it);
    mexErrMsgTxt(landing_last_error());
  }
  {
    mxArray* out[7] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL};
    out[0] = mxCreateDoubleMatrix((mwSize)nxk, (mwSize)B, mxREAL); memcpy(mxGetPr(out[0]), X, (size_t)nxk * B * sizeof(double));
    if (nlhs > 1) { out[1] = mxCreateDoubleMatrix(1, (mwSize)B, mxREAL); memcpy(mxGetPr(out[1]), F, (size_t)B * sizeof(double)); }
    if (nlhs > 2) { out[2] = mxCreateNumericMatrix(3, (mwSize)B, mxINT32_CLASS, mxREAL); memcpy(mxGetData(out[2]), st, 3 * (size_t)B * sizeof(int)); }
    if (nlhs > 3) { out[3] = mxCreateNumericMatrix(3, (mwSize)B, mxINT32_CLASS, mxREAL); memcpy(mxGetData(out[3]), it, 3 * (size_t)B * sizeof(int)); }
    if (nlhs > 4) { out[4] = mxCreateDoubleMatrix(3, (mwSize)B, mxREAL); memcpy(mxGetPr(out[4]), KK, 3 * (size_t)B * sizeof(double)); }
    if (nlhs > 5) { out[5] = mxCreateDoubleMatrix(9, (mwSize)kept, mxREAL); memcpy(mxGetPr(out[5]), pin, 9 * (size_t)kept * sizeof(double)); }
    if (nlhs > 6) { out[6] = mxCreateDoubleMatrix((mwSize)nxk, (mwSize)kept, mxREAL); memcpy(mxGetPr(out[6]), pout, (size_t)nxk * kept * sizeof(double)); }
    mxFree(X); mxFree(F); mxFree(KK); mxFree(pin); mxFree(pout); mxFree(st); mxFree(it);
    for (i = 0; i < 7; ++i) if (i < (nlhs > 1 ? nlhs : 1)) plhs[i] = out[i];
  }
}
