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

// R = U*diag(1,1,det(U*V'))*V' for the 3x3 block M (row-major)  (Spectral.m:43-45); host only.
// One-sided (Hestenes) Jacobi SVD of M itself: column rotations make the columns of G = M V orthogonal, their norms are the singular
// values.  M'M is never formed, so a small singular value is not lost under the square of the largest (U = M v / sqrt(eig(M'M)) left
// RR' - I at eps * cond(M)^2 and never saw a rank-deficient block as one).  The third left vector does not need sigma_3:
// R = u1 v1' + u2 v2' + det(V) (u1 x u2) v3', with u2 re-orthogonalised against u1; a block of rank 1 gets a u2 completed from the
// coordinate axis farthest from u1, the zero block the identity (svd(0): U = V = I).
inline void project_so3(const double* M, double* R) {
    double big = 0.0;
    for (int t = 0; t < 9; ++t) big = std::max(big, std::fabs(M[t]));
    if (!(big > 0.0)) { for (int t = 0; t < 9; ++t) R[t] = (t % 4 == 0); return; }
    int ex = 0;
    (void)std::frexp(big, &ex);                                   // entries scaled by a power of two into [-1, 1]: no overflow at 1e+-100
    double G[3][3], V[3][3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { G[r][c] = std::ldexp(M[r * 3 + c], -ex); V[r][c] = r == c; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int k = 0; k < 3; ++k) { al += G[k][p] * G[k][p]; be += G[k][q] * G[k][q]; ga += G[k][p] * G[k][q]; }
                if (!(std::fabs(ga) > 1.1102230246251565e-16 * std::sqrt(al) * std::sqrt(be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double gp = G[k][p], gq = G[k][q]; G[k][p] = c * gp - s * gq; G[k][q] = s * gp + c * gq;
                    const double vp = V[k][p], vq = V[k][q]; V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double sv[3];
    for (int c = 0; c < 3; ++c) sv[c] = std::sqrt(G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c]);
    int idx[3];                                                   // descending, equal values keep their index order
    for (int i = 0; i < 3; ++i) { int j = i; for (; j > 0 && sv[i] > sv[idx[j - 1]]; --j) idx[j] = idx[j - 1]; idx[j] = i; }
    auto unit = [](double* a) { const double nr = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); for (int k = 0; k < 3; ++k) a[k] /= nr; return nr; };
    double u1[3], u2[3], u3[3], v[3][3];                          // v[c]: right vector c
    for (int c = 0; c < 3; ++c) {
        for (int k = 0; k < 3; ++k) v[c][k] = V[k][idx[c]];
        unit(v[c]);                                               // the accumulated rotations leave a few eps
    }
    for (int k = 0; k < 3; ++k) { u1[k] = G[k][idx[0]]; u2[k] = G[k][idx[1]]; }
    unit(u1);
    bool have2 = sv[idx[1]] > 0.0;
    if (have2) {
        unit(u2);
        const double d = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
        for (int k = 0; k < 3; ++k) u2[k] -= d * u1[k];
        have2 = unit(u2) > 0.5;
    }
    if (!have2) {                                                 // rank 1: complete an orthonormal basis
        const int k = std::fabs(u1[0]) < std::fabs(u1[1]) ? (std::fabs(u1[0]) < std::fabs(u1[2]) ? 0 : 2) : (std::fabs(u1[1]) < std::fabs(u1[2]) ? 1 : 2);
        double e[3] = {0, 0, 0}; e[k] = 1;
        u2[0] = u1[1] * e[2] - u1[2] * e[1]; u2[1] = u1[2] * e[0] - u1[0] * e[2]; u2[2] = u1[0] * e[1] - u1[1] * e[0];
        unit(u2);
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    unit(u3);
    const double detV = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                        v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    const double d = detV < 0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = u1[r] * v[0][c] + u2[r] * v[1][c] + d * u3[r] * v[2][c];
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
