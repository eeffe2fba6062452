// chol.h -- device-resident blocked Cholesky object (see chol.hip)
#pragma once
#include "hdm_common.h"
#include <vector>

struct HdmChol {
    int n = 0, npad = 0, nblk = 0;
    HdmBuf<double> L;        // npad x npad, column-major; lower triangle = Cholesky factor after factor()
    HdmBuf<double> Linv;     // npad x npad, lower triangular inverse (explicit zeros above the diagonal)
    HdmBuf<double> Dinv;     // nblk x (128 x 128) inverted diagonal blocks
    HdmBuf<double> Z;        // npad x 128 scratch for invert_factor
    HdmBuf<double> Zd;       // npad x npad scratch for the recursive-doubling variant of invert_factor
    HdmBuf<double> vec;      // 4 * npad scratch vectors
    HdmBuf<int> info_dev;
    bool factored = false, have_inv = false;
    bool logdet_ok = false;  // log det of the factored matrix is known (single-launch small-block check): 2 sum log L_kk
    double logdet_val = 0.0;
    // single-launch block substitution (hdm_trsv_flow_kernel): per (rhs, direction, block) publication flags + error word
    HdmBuf<int> flow_flags;
    HdmPinned<int> flow_err;     // mapped host word: a workgroup gave up waiting
    int flow_epoch = 0;
    bool flow_ok = true, flow_pending = false;
    int flow_cap = -1;           // co-residency bound on this object's device (workgroups), computed at the first solve
    std::vector<double> host_stage;   // solve_host: solutions land here first (in-place solves, retry after a give-up)
    // Block envelope of a matrix with structural zeros (the sparse Schur operator's M): env_first[i] = first 128-block column
    // with an entry in block row i, env_colh[k] = last block row whose envelope reaches block column k (non-decreasing).
    // A Cholesky factor fills inside the row envelope only, so the factorisation's panel and trailing update of block column k
    // stop at row env_colh[k] and the substitutions skip the blocks outside.  Empty = dense.
    std::vector<int> env_first, env_colh;
    HdmBuf<int> env_dev;         // device copy: first[nblk], then colh[nblk]
    // factor_signed (KKT_TYPE_PRIMAL with an indefinite X): the pivot signs and two info words of the last signed factorisation
    HdmBuf<double> sgn;          // npad: sign of pivot k (+1 in the identity padding)
    HdmBuf<int> sinfo_dev;       // [0] first zero / non-finite pivot + 1, [1] negative pivots

    int init(int n);
    int set_envelope(const int *first_blockcol_of_blockrow);   // nblk entries; nullptr = dense.  Before the first factor().
    int load_host(const double *A, long lda, hipStream_t s);
    int load_device(const double *A, long lda, hipStream_t s);
    int finish_load(hipStream_t s);
    int factor(hipStream_t s, int *info_host);          // info = 0 ok, j+1 = first non-positive pivot
    int invert_factor(hipStream_t s);                   // builds Linv (idempotent until the next load)
    int set_reverse_inverse(hipStream_t s);             // primal builds: Linv <- W, W^T W = X, from the factor of J X J
    // blocked LDL' without pivoting in Cholesky clothing (the SIGNED sweep of sweep128.h per diagonal block): A = F S F^T,
    // S = diag(sgn), F lower with a positive diagonal.  info = first exactly zero / non-finite pivot + 1 (0: factored),
    // nneg = negative pivots.  After it, set_reverse_inverse gives W with W^T diag(sigma) W = X, sigma from reverse_signs.
    int factor_signed(hipStream_t s, int *info_host, int *nneg_host);
    int reverse_signs(double *sig_dev, hipStream_t s);  // sig[i] = sgn[n - 1 - i] for i < n, +1 in the padding (npad entries)
    int get_diag(double *diag_host, hipStream_t s);
    int solve_device(double *b_dev, double *x_dev, int nrhs, long ldv, int which, hipStream_t s);
    int solve_host(const double *rhs, double *sol, int nrhs, int which, hipStream_t s);
    // after the synchronisation that follows solve_device: did a workgroup of the single-launch substitution give up waiting?
    // Then its result is to be thrown away; later solves use per-block launches.  (Reads and clears the give-up word.)
    bool flow_gave_up();
    int inverse_full(double *out_dev, long ldo, hipStream_t s);
};

// diagonal-tile factorisations of a block-sparse matrix (bsparse.hip): 128 x 128 tiles, 16384 doubles apart; tile
// diag_tile[cols[b]] is factored in place (lower), its inverse goes to Winv + cols[b] * 16384; rows past m are padding
int hdm_potrf_sweep_configure();
// sgn == nullptr: Cholesky sweeps (info[0] = first non-positive pivot + 1).  sgn != nullptr: the signed LDL' sweep of sweep128.h --
// sgn[128 k ..] <- pivot signs of block column k, info[0] = first zero / non-finite pivot + 1, info[1] += negative pivots
int hdm_potrf_sweep_batched(double *tiles, const int *diag_tile, const int *cols, int ncols, double *Winv, int *info, int m, hipStream_t s,
                            double *sgn = nullptr);

// several engine shards share this device: the single-launch substitution (which needs co-resident workgroups) is off
void hdm_flow_set_shared_device(int on);
bool hdm_flow_shared_device();   // several engine instances share one device: no kernel may count on its grid being co-resident
double hdm_diag_block_probe(int variant, int reps, hipStream_t s);   // diagnostic: us per diagonal-block kernel (0: LDS panels, 1: register sweep)
