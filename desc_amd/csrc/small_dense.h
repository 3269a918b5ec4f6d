// Small dense helpers of the Spectral / GCW eigen-solve, shared by spectral.hip (one problem per call: they run on the host between
// launches) and gcw_batch.hip (many small problems per launch: they run inside the kernel).  Both files must do the same arithmetic
// on the same inputs, so the text lives here once.
#pragma once
#include <algorithm>
#include <cmath>

#include <hip/hip_runtime.h>

namespace desc {

// cyclic Jacobi eigen-decomposition of a symmetric N x N matrix (row-major); eigenvalues
// descending in w, eigenvectors in the columns of V
template <int N>
__host__ __device__ inline void jacobi_eig(const double* Ain, double* w, double* V) {
    double A[N][N];
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) { A[i][j] = 0.5 * (Ain[i * N + j] + Ain[j * N + i]); V[i * N + j] = i == j; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < N; ++p) for (int q = p + 1; q < N; ++q) off += A[p][q] * A[p][q];
        if (off < 1e-300) break;
        for (int p = 0; p < N; ++p)
            for (int q = p + 1; q < N; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                for (int k = 0; k < N; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                for (int k = 0; k < N; ++k) { const double vkp = V[k * N + p], vkq = V[k * N + q]; V[k * N + p] = c * vkp - s * vkq; V[k * N + q] = s * vkp + c * vkq; }
            }
    }
    // descending by eigenvalue; a stable insertion sort (equal values keep their index order)
    int idx[N];
    for (int i = 0; i < N; ++i) {
        int j = i;
        for (; j > 0 && A[i][i] > A[idx[j - 1]][idx[j - 1]]; --j) idx[j] = idx[j - 1];
        idx[j] = i;
    }
    double Vs[N * N];
    for (int c = 0; c < N; ++c) { w[c] = A[idx[c]][idx[c]]; for (int k = 0; k < N; ++k) Vs[k * N + c] = V[k * N + idx[c]]; }
    for (int t = 0; t < N * N; ++t) V[t] = Vs[t];
}

// C = Z * L^-T where K = Z' G Z = L L'  (columns of Y*C are orthonormal when G = Y'Y); all N x N row-major.
// false: K is not positive definite in double precision (rank-deficient block)
template <int N>
__host__ __device__ inline bool ortho_coeffs(const double* G, const double* Z, double* C) {
    double K[N][N], L[N][N] = {};
    for (int a = 0; a < N; ++a) for (int b = 0; b < N; ++b) { double s = 0; for (int p = 0; p < N; ++p) for (int q = 0; q < N; ++q) s += Z[p * N + a] * G[p * N + q] * Z[q * N + b]; K[a][b] = s; }
    for (int a = 0; a < N; ++a) {
        for (int b = 0; b <= a; ++b) {
            double s = 0.5 * (K[a][b] + K[b][a]);
            for (int k = 0; k < b; ++k) s -= L[a][k] * L[b][k];
            if (a == b) { if (!(s > 0)) return false; L[a][a] = sqrt(s); } else L[a][b] = s / L[b][b];
        }
    }
    // Linv' : solve L' X = I  -> X = L^-T ; then C = Z X
    double Li[N][N] = {};
    for (int c = 0; c < N; ++c)
        for (int r = N - 1; r >= 0; --r) { double s = (r == c); for (int k = r + 1; k < N; ++k) s -= L[k][r] * Li[k][c]; Li[r][c] = s / L[r][r]; }
    for (int a = 0; a < N; ++a) for (int b = 0; b < N; ++b) { double s = 0; for (int k = 0; k < N; ++k) s += Z[a * N + k] * Li[k][b]; C[a * N + b] = s; }
    return true;
}

// R = U*diag(1,1,det(U*V'))*V' for the 3x3 block M (row-major)  (Spectral.m:43-45); host only
inline void project_so3(const double* M, double* R) {
    // eigen-decomposition of M'M gives V and the singular values; U = M V / sigma
    double MtM[9], w[3], V[9];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { double s = 0; for (int k = 0; k < 3; ++k) s += M[k * 3 + a] * M[k * 3 + b]; MtM[a * 3 + b] = s; }
    jacobi_eig<3>(MtM, w, V);
    double U[9];
    const double s0 = std::sqrt(std::max(w[0], 0.0));
    int good = 0;
    for (int c = 0; c < 3; ++c) {
        const double sc = std::sqrt(std::max(w[c], 0.0));
        if (sc > 1e-12 * std::max(s0, 1e-300) && sc > 1e-300) {
            for (int r = 0; r < 3; ++r) { double s = 0; for (int k = 0; k < 3; ++k) s += M[r * 3 + k] * V[k * 3 + c]; U[r * 3 + c] = s / sc; }
            good = c + 1;
        } else break;
    }
    if (good == 0) { for (int i = 0; i < 9; ++i) { U[i] = (i % 4 == 0); V[i] = (i % 4 == 0); } good = 3; }   // svd(0): U = V = I
    if (good == 1) {      // complete an orthonormal basis
        double a[3] = {U[0], U[3], U[6]}; int k = std::fabs(a[0]) < std::fabs(a[1]) ? (std::fabs(a[0]) < std::fabs(a[2]) ? 0 : 2) : (std::fabs(a[1]) < std::fabs(a[2]) ? 1 : 2);
        double e[3] = {0, 0, 0}; e[k] = 1;
        double b[3] = {a[1] * e[2] - a[2] * e[1], a[2] * e[0] - a[0] * e[2], a[0] * e[1] - a[1] * e[0]};
        const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
        for (int r = 0; r < 3; ++r) U[r * 3 + 1] = b[r] / nb;
        good = 2;
    }
    if (good == 2) {
        const double a[3] = {U[0], U[3], U[6]}, b[3] = {U[1], U[4], U[7]};
        U[2] = a[1] * b[2] - a[2] * b[1]; U[5] = a[2] * b[0] - a[0] * b[2]; U[8] = a[0] * b[1] - a[1] * b[0];
    }
    auto det3 = [](const double* A) { return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]); };
    double UVt[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { double s = 0; for (int k = 0; k < 3; ++k) s += U[r * 3 + k] * V[c * 3 + k]; UVt[r * 3 + c] = s; }
    const double d = det3(UVt) < 0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = U[r * 3 + 0] * V[c * 3 + 0] + U[r * 3 + 1] * V[c * 3 + 1] + d * U[r * 3 + 2] * V[c * 3 + 2];
}

// The tail of the eigen-solve for one problem on the host, the arithmetic of spectral.hip's (Spectral.m:39-46 / GCW.m:21,27-36).
// ritz_scale_sign: V holds the three Ritz vectors (3n x 3, row-major), dinv the D^-1/2 they are scaled back with (NULL: no row
// normalisation); V becomes the eigenvectors of D^-1 A with unit 2-norm columns (what eigs returns), V(:,1) = V(:,1)*sign(det(V(1:3,:))).
// project_nodes: the per-node SVD projection of nodes v0 .. v1 into R_out (3x3xn, MATLAB column-major).
inline void ritz_scale_sign(double* V, const double* dinv, int64_t n) {
    const int64_t rows = 3 * n;
    double nrm[3] = {0, 0, 0};
    for (int64_t v = 0; v < n; ++v) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) {
        const double x = V[((size_t)3 * v + r) * 3 + c] * (dinv ? dinv[v] : 1.0);
        V[((size_t)3 * v + r) * 3 + c] = x; nrm[c] += x * x;
    }
    for (size_t t = 0; t < (size_t)rows * 3; ++t) V[t] /= std::sqrt(nrm[t % 3]);
    const double* A = V;
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    const double sg = det > 0 ? 1.0 : (det < 0 ? -1.0 : 0.0);
    for (int64_t r = 0; r < rows; ++r) V[(size_t)r * 3] *= sg;
}
inline void project_nodes(const double* V, int64_t v0, int64_t v1, double* R_out) {
    for (int64_t v = v0; v < v1; ++v) {
        double R[9];
        project_so3(&V[(size_t)9 * v], R);           // rows 3v..3v+2 of V = the node's 3x3 block, row-major
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R_out[9 * v + r + 3 * c] = R[r * 3 + c];   // MATLAB column-major 3x3xn
    }
}

}  // namespace desc
