// Horn's closed-form absolute orientation (Jigsaw_matching/utils/pairwise_alignment.py:11-79) on the device, shared by the rigid
// term of the training loss (matching_rigid.hip) and the evaluation's pairwise RANSAC (matching_pose.hip): the 4 x 4 matrix N of
// the 3 x 3 correlation M, its eigenvectors by a cyclic Jacobi in fp64, and the rotation of a unit quaternion.  Every expression
// keeps the order of the reference's formulas; the units that include this are compiled with -ffp-contract=off.
#pragma once

constexpr int RG_SWEEPS = 10;        // cyclic Jacobi sweeps on the 4 x 4: quadratic convergence, six suffice in fp64

// one Jacobi rotation of the symmetric A (full storage) in the plane (P_, Q_), accumulated into the eigenvector matrix V
template <int P_, int Q_>
__device__ __forceinline__ void rg_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P_][Q_];
  if (apq == 0.0) return;
  const double theta = (A[Q_][Q_] - A[P_][P_]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                      // columns P_, Q_ of A and of V
    const double akp = A[k][P_], akq = A[k][Q_];
    A[k][P_] = c * akp - s * akq;
    A[k][Q_] = s * akp + c * akq;
    const double vkp = V[k][P_], vkq = V[k][Q_];
    V[k][P_] = c * vkp - s * vkq;
    V[k][Q_] = s * vkp + c * vkq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                      // rows P_, Q_ of A
    const double apk = A[P_][k], aqk = A[Q_][k];
    A[P_][k] = c * apk - s * aqk;
    A[Q_][k] = s * apk + c * aqk;
  }
  A[P_][Q_] = 0.0;
  A[Q_][P_] = 0.0;
}

// Horn's N (pairwise_alignment.py:20-47) of M = sum (S - cS) (T - cT)^T
__device__ __forceinline__ void rg_horn_n(const double (&M)[3][3], double (&A)[4][4]) {
  A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  A[2][2] = (M[1][1] - M[0][0]) - M[2][2];
  A[3][3] = (M[2][2] - M[0][0]) - M[1][1];
  A[0][1] = A[1][0] = M[1][2] - M[2][1];
  A[0][2] = A[2][0] = M[2][0] - M[0][2];
  A[0][3] = A[3][0] = M[0][1] - M[1][0];
  A[1][2] = A[2][1] = M[0][1] + M[1][0];
  A[1][3] = A[3][1] = M[0][2] + M[2][0];
  A[2][3] = A[3][2] = M[1][2] + M[2][1];
}

// the eigenvalues ev (unsorted: the diagonal Jacobi leaves) of A, which is destroyed, and the eigenvector qv of the FIRST of the
// largest, whose index is returned; V is scratch.  A = 0 gives qv = (1, 0, 0, 0): the identity rotation, as LAPACK does for the reference
__device__ __forceinline__ int rg_top_eigenvector(double (&A)[4][4], double (&V)[4][4], double (&ev)[4], double (&qv)[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[a][c] = a == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < RG_SWEEPS; ++sweep) {
    rg_rotate<0, 1>(A, V); rg_rotate<0, 2>(A, V); rg_rotate<0, 3>(A, V);
    rg_rotate<1, 2>(A, V); rg_rotate<1, 3>(A, V); rg_rotate<2, 3>(A, V);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ev[k] = A[k][k];
    qv[k] = V[k][0];
  }
  double best = ev[0];
  int kb = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    if (ev[k] > best) {                                              // strict: the first of equal maxima
      best = ev[k];
      kb = k;
#pragma unroll
      for (int a = 0; a < 4; ++a) qv[a] = V[a][k];
    }
  }
  return kb;
}

// the rotation of the unit quaternion qv (pairwise_alignment.py:52-70)
__device__ __forceinline__ void rg_quat_rot(const double (&qv)[4], double (&Rd)[3][3]) {
  const double q0 = qv[0], q1 = qv[1], q2 = qv[2], q3 = qv[3];
  Rd[0][0] = ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3;
  Rd[0][1] = 2.0 * (q1 * q2 - q0 * q3);
  Rd[0][2] = 2.0 * (q1 * q3 + q0 * q2);
  Rd[1][0] = 2.0 * (q2 * q1 + q0 * q3);
  Rd[1][1] = ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3;
  Rd[1][2] = 2.0 * (q2 * q3 - q0 * q1);
  Rd[2][0] = 2.0 * (q3 * q1 - q0 * q2);
  Rd[2][1] = 2.0 * (q3 * q2 + q0 * q1);
  Rd[2][2] = ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3;
}
