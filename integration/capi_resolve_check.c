/* capi_resolve_check.c — a plain C client of the reference's C API (highs/interfaces/highs_c_api.h) that solves a model,
 * changes it and solves again, the way a long-lived HiGHS user does: Highs_changeColCost, Highs_changeCoeff on an
 * existing entry, Highs_changeRowBounds that changes a row's kind, Highs_run after each.  Nothing here knows about the
 * GPU.  With PDLP_MI355X_KEEP_SOLVER=1 in the environment the drop-in wrapper (CupdlpWrapperMi355x.cpp) keeps one
 * resident solver across the runs (pdlp_mi355x_session_solve) instead of setting one up per run; the lines printed here
 * must not depend on that, to the last digit.
 * Usage: capi_resolve_check model-file [kkt_tolerance [output_flag]]
 * Prints one line per run: model status, objective, pdlp_iteration_count, first and last column value.
 * Exit code 0 = all four runs returned without an error. */
#include <stdio.h>
#include <stdlib.h>

#include "interfaces/highs_c_api.h"

static int run_and_print(void* h, int k, const char* what) {
  const HighsInt rs = Highs_run(h);
  const HighsInt ms = Highs_getModelStatus(h);
  const HighsInt nc = Highs_getNumCol(h), nr = Highs_getNumRow(h);
  double* cv = (double*)calloc((size_t)(nc > 0 ? nc : 1), sizeof(double));
  double* cd = (double*)calloc((size_t)(nc > 0 ? nc : 1), sizeof(double));
  double* rv = (double*)calloc((size_t)(nr > 0 ? nr : 1), sizeof(double));
  double* rd = (double*)calloc((size_t)(nr > 0 ? nr : 1), sizeof(double));
  Highs_getSolution(h, cv, cd, rv, rd);
  HighsInt it = -1;
  Highs_getIntInfoValue(h, "pdlp_iteration_count", &it);
  printf("capi_resolve_check: run=%d (%s) model_status=%d objective=%.17g pdlp_iteration_count=%d x_first=%.17g x_last=%.17g\n", k, what,
         (int)ms, Highs_getObjectiveValue(h), (int)it, cv[0], cv[nc > 0 ? nc - 1 : 0]);
  fflush(stdout);
  free(cv); free(cd); free(rv); free(rd);
  return rs == kHighsStatusError ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: capi_resolve_check model-file [kkt_tolerance [output_flag]]\n");
    return 2;
  }
  void* h = Highs_create();
  if (!h) return 2;
  Highs_setBoolOptionValue(h, "output_flag", argc > 3 ? atoi(argv[3]) : 0);
  if (Highs_setStringOptionValue(h, "solver", "pdlp") != kHighsStatusOk) return 3;
  Highs_setStringOptionValue(h, "presolve", "off");
  Highs_setDoubleOptionValue(h, "kkt_tolerance", argc > 2 ? atof(argv[2]) : 1e-6);
  if (Highs_readModel(h, argv[1]) == kHighsStatusError) return 4;
  const HighsInt nc = Highs_getNumCol(h), nr = Highs_getNumRow(h), nz = Highs_getNumNz(h);
  if (nc < 1 || nr < 1 || nz < 1) return 5;
  const double inf = Highs_getInfinity(h);
  int bad = 0;

  bad |= run_and_print(h, 1, "as read");

  /* the model as HiGHS holds it */
  double* cost = (double*)malloc(sizeof(double) * (size_t)nc);
  double* clo = (double*)malloc(sizeof(double) * (size_t)nc);
  double* cup = (double*)malloc(sizeof(double) * (size_t)nc);
  HighsInt* start = (HighsInt*)malloc(sizeof(HighsInt) * (size_t)(nc + 1));
  HighsInt* index = (HighsInt*)malloc(sizeof(HighsInt) * (size_t)nz);
  double* value = (double*)malloc(sizeof(double) * (size_t)nz);
  HighsInt got_col = 0, got_nz = 0;
  if (Highs_getColsByRange(h, 0, nc - 1, &got_col, cost, clo, cup, &got_nz, start, index, value) != kHighsStatusOk || got_col != nc) return 6;
  start[nc] = got_nz;

  /* some column costs */
  for (HighsInt j = 0; j < nc && j < 5; ++j)
    if (Highs_changeColCost(h, j, cost[j] * 1.25 + 0.5) != kHighsStatusOk) return 7;
  bad |= run_and_print(h, 2, "column costs changed");

  /* a coefficient on an existing entry: the first entry of the first column that has one */
  HighsInt col = 0;
  while (col < nc && start[col + 1] == start[col]) ++col;
  if (col == nc) return 8;
  if (Highs_changeCoeff(h, index[start[col]], col, value[start[col]] * 1.5) != kHighsStatusOk) return 8;
  bad |= run_and_print(h, 3, "coefficient changed");

  /* a row bound that changes the row's kind: the first equality becomes <=, else the first one-sided row an equality */
  double* rlo = (double*)malloc(sizeof(double) * (size_t)nr);
  double* rup = (double*)malloc(sizeof(double) * (size_t)nr);
  HighsInt got_row = 0, row_nz = 0;
  if (Highs_getRowsByRange(h, 0, nr - 1, &got_row, rlo, rup, &row_nz, NULL, NULL, NULL) != kHighsStatusOk || got_row != nr) return 9;
  HighsInt row = -1;
  for (HighsInt i = 0; i < nr && row < 0; ++i)
    if (rlo[i] == rup[i] && rlo[i] > -inf && rup[i] < inf) row = i;
  if (row >= 0) {
    if (Highs_changeRowBounds(h, row, -inf, rup[row]) != kHighsStatusOk) return 10;
  } else {
    for (HighsInt i = 0; i < nr && row < 0; ++i)
      if ((rlo[i] > -inf) != (rup[i] < inf)) row = i;
    if (row < 0) return 10;
    const double v = rlo[row] > -inf ? rlo[row] : rup[row];
    if (Highs_changeRowBounds(h, row, v, v) != kHighsStatusOk) return 10;
  }
  bad |= run_and_print(h, 4, "row kind changed");

  free(cost); free(clo); free(cup); free(start); free(index); free(value); free(rlo); free(rup);
  Highs_destroy(h);
  return bad ? 20 : 0;
}
