// The rotation of the similarity alignment (eval.py:110-161) without a library solver: Horn's closed form.  The proper
// rotation R that maximises tr(R K), K = X1 X2^T, is the one of the unit quaternion that is the eigenvector of the largest
// eigenvalue of a symmetric 4 x 4 matrix N(K) (B. K. P. Horn, "Closed-form solution of absolute orientation using unit
// quaternions", J. Opt. Soc. Am. A 4, 1987).  It is the reference's V diag(1, 1, sign det(U V^T)) U^T: the eigenvalues of N
// are s1+s2+s3', s1-s2-s3', -s1+s2-s3', -s1-s2+s3' with s3' = sign(det K) s3, so the maximiser is unique exactly when
// s2 + s3' > 0, and a mirrored or planar point set needs no special case.  N is diagonalised by cyclic Jacobi rotations in
// fp64; every index is a compile-time constant, so the matrices live in registers.
#pragma once
#include <math.h>

namespace scat {

template <int P, int Q>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    // the smaller root of t^2 + 2 t theta - 1 = 0; theta^2 may overflow to inf, which gives t = 0 as it should
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// K row-major, K[3 a + c] = sum_j X1[a][j] X2[c][j]  ->  R row-major
__host__ __device__ inline void horn_rotation(const double* K, double* R) {
    const double Sxx = K[0], Sxy = K[1], Sxz = K[2], Syx = K[3], Syy = K[4], Syz = K[5], Szx = K[6], Szy = K[7], Szz = K[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    double frob = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) frob += A[i][j] * A[i][j];
    // quadratic convergence: the off-diagonal part falls below the rounding of the diagonal within 6 sweeps or so; the
    // bound of 16 only keeps a matrix of NaNs from looping
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] +
                           A[1][3] * A[1][3] + A[2][3] * A[2][3];
        if (!(off > 1e-36 * frob)) break;
        jacobi_rotate<0, 1>(A, V);
        jacobi_rotate<0, 2>(A, V);
        jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V);
        jacobi_rotate<1, 3>(A, V);
        jacobi_rotate<2, 3>(A, V);
    }
    double lam = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const bool up = A[i][i] > lam;
        lam = up ? A[i][i] : lam;
        w = up ? V[0][i] : w;
        x = up ? V[1][i] : x;
        y = up ? V[2][i] : y;
        z = up ? V[3][i] : z;
    }
    const double n = 1.0 / sqrt(w * w + x * x + y * y + z * z);   // V is orthogonal to rounding; this takes the rounding out
    w *= n;
    x *= n;
    y *= n;
    z *= n;
    R[0] = w * w + x * x - y * y - z * z;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = w * w - x * x + y * y - z * z;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = w * w - x * x - y * y + z * z;
}

}  // namespace scat
