// Launchers that one kernel file defines and another calls: the round driver (round.hip) queues the kernels of
// msm.hip, ml.hip and gather.hip directly, and ml.hip's selection sets the speculative rows' flags through
// msm.hip.  The caller and the defining file both include this header, so a prototype that drifts from its
// definition is a compile error (conflicting declarations of a C-linkage function) instead of silently
// misplaced arguments.  Only what crosses files belongs here; the Python-facing ABI is ops/_abi.py.
#pragma once
#include <stdint.h>

#define ROWARG_MAX 248   // rows the share MSM takes in its kernel arguments (msm.hip RowArg, bsc_shares_msm_ka)

extern "C" {
// msm.hip
int bsc_shares_msm(const long long* coeffs, int d, const int* rows, int nrows, const uint32_t* tbl_pk,
                   const uint32_t* tbl_wb, int poly, int T, int B0, int NW, int commit_only, const int* alive,
                   const int* compact, int group_rows, uint32_t* out_pts, long long* out_y, void* stream);
int bsc_shares_msm_ka(const long long* coeffs, int d, const int* rows_host, int nrows, const uint32_t* tbl_pk,
                      const uint32_t* tbl_wb, int poly, int T, int B0, int NW, int commit_only, const int* alive,
                      int group_rows, uint32_t* out_pts, long long* out_y, void* stream);
int bsc_set_alive(const int* accept, const int* src, int n, int* alive, void* stream);
int bsc_sum_rows2(const uint32_t* pts, int ncols_in, const int* rows, int nrows, const int* cols, int ncols,
                  const int* row_mask, int mask_by_pos, uint32_t* out, void* stream);
int bsc_sum_cols_serial(const uint32_t* pts, int ncols_in, int nrows, const int* cols, int ncols,
                        const int* row_mask, uint32_t* out, void* stream);
int bsc_segment_sum(const uint32_t* pts, int ngroups, int n, int stride, int off, uint32_t* out, uint32_t* hout,
                    void* stream);
int bsc_chunk_check(const long long* coeffs, int d, int poly, const uint32_t* tbl_pk, int B0, int NW,
                    const uint32_t* csum, int nm, int nch, int* ok, int* h_ok, void* stream);
int bsc_g1_unmarshal(const uint8_t* in, int n, const int* pre, uint32_t* out, int* valid, void* stream);
int bsc_chain_audit(const double* models, const int* kind, const int* offsets, int L, int d, const double* plain,
                    const int* pbeg, const int* pend, int np, const uint8_t* commits, const int* len_ok, int n,
                    const uint32_t* tbl_pk, int B0, int NW, double scale, double tol, double wmax, int slab,
                    long long* coeffs, const int* rows, uint32_t* partial, uint32_t* msm, uint32_t* aff, int* valid,
                    int* res, int* h_res, void* stream);
int bsc_wave_prio_msm(int on);
// ml.hip
int bsc_softmax_step(const float* X, const int* y, const long long* off, const int* ntrain, const int* pid,
                     const double* W, int D_IN, int D_OUT, int B, int P, unsigned long long seed, int iteration,
                     float max_norm, double qscale, float* delta, long long* qdelta, float* loss, int lo, int* ones,
                     int nones, void* stream);
int bsc_margin_step(const float* X, const int* y, const long long* off, const int* ntrain, const int* pid,
                    const double* W, int D_IN, int D_OUT, int B, int P, unsigned long long seed, int iteration,
                    float max_norm, double qscale, float* delta, long long* qdelta, float* loss, int lo, int* ones,
                    int nones, void* stream);
int bsc_gram_stacked_range(const float* X, int U1, const float* X2, int U2, long long stride2, int D, int kchunk,
                           int p0, int p1, double* part, double* gram, unsigned int* count, const double* nn,
                           void* stream);
int bsc_sum_rows_i64_tail(const long long* ys, int R, long long C, const int* mask, long long* out, long long tail,
                          void* stream);
int bsc_recover_w_clock(const long long* ys, int nrows, long long rstride, int nch, int T, const int* mask,
                        const int* ycols, const int* xs, int npts, const long long* A, const int* basis, int poly,
                        int shift, unsigned long long inv_lo, unsigned long long inv_hi, int d, const double* W,
                        double qscale, double* W_new, long long* coeffs, int* status, long long* agg_out, double* h_W,
                        int* h_status, long long* h_clock, void* stream);
int bsc_wave_prio_ml(int on);
// gather.hip
int bsc_vg_pack(uint8_t* row, long long commit_off, long long nz_off, long long sc_off, const uint32_t* commits,
                int maxlocal, int pw, const int* src_row, const int* nz, const float* sc, int nnz, void* stream);
int bsc_vg_unpack(const uint8_t* recv, long long row_bytes, int chunk, int npairs, long long commit_off,
                  long long nz_off, long long sc_off, int maxlocal, int pw, int nn, int world, const int* wrow, int nw,
                  double* gram, int* nz, float* sc, uint32_t* commits_host, void* stream);
// vrf.hip
int bsc_wave_prio_vrf(int on);
}
