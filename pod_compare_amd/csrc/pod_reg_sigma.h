// What the evaluation's regression scoring rules share (k_reg_nll of k5_cluster_merge.hip, k33_eval_scores.hip): Sigma = cov + 1e-2 I of one
// row and its Cholesky factor -- one copy, so that the NLL, the energy score and the CRPS of a detection see the same factor.
#pragma once

#include "pod_device.h"

namespace pod {

// cov: the row's 16 floats.  Sigma = cov + 1e-2 I is formed in fp32 (scoring_rules.py:68 forms it so) and widened; L L^T = Sigma in fp64,
// the lower triangle read, the strict upper triangle of L left unwritten.  A Sigma that is not positive definite leaves NaN (or a zero) on
// L's diagonal: reg_sigma_ok.
__device__ __forceinline__ void reg_sigma_factor(const float* cov, double (&a)[4][4], double (&L)[4][4]) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) a[r][c] = (double)(cov[r * 4 + c] + ((r == c) ? 1e-2f : 0.0f));
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c <= r; ++c) {
            double s = a[r][c];
            for (int k = 0; k < c; ++k) s -= L[r][k] * L[c][k];
            if (r == c) {
                L[r][r] = sqrt(s);
            } else {
                L[r][c] = s / L[c][c];
            }
        }
}

__device__ __forceinline__ bool reg_sigma_ok(const double (&L)[4][4]) {
    return L[0][0] > 0.0 && L[1][1] > 0.0 && L[2][2] > 0.0 && L[3][3] > 0.0;      // false for NaN
}

}  // namespace pod
