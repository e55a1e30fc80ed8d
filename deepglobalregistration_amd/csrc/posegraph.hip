// Robust pose-graph optimisation with line processes (Choi, Zhou, Koltun 2015; the step Open3D's global_optimization runs
// on a scene's .log + .info): one pose per fragment in a common frame from the registered, scored pairs of a scene.
//
// Definition (float64 throughout).  Edge e = (s, t, X, Lambda, uncertain): X the pose of s in t's frame,
// Lambda the pair's 6x6 information matrix (rotation block first).  E = inv(P_t) P_s inv(X), xi = (rotation vector of E,
// translation of E), chi2 = xi^T Lambda xi -- pg_residual below is the ONE device statement of the residual
// (core/pose_graph.py: edge_residuals is its host twin).  The solver minimises
//     F*(P) = sum_certain chi2 + sum_uncertain mu chi2 / (mu + chi2)
// by Levenberg-Marquardt with the line-process weights l = (mu / (mu + chi2))^2 recomputed at every outer iteration and
// frozen inside it; a step is judged on the frozen-weight objective sum l chi2 + mu (sqrt(l) - 1)^2, which majorises F*
// and touches it at the current poses, so F* never increases.
//
// One workgroup per graph (blockIdx.x), one persistent kernel, no host round trip between iterations.  Per iteration:
//   1. edge pass (thread = edge): E, xi, chi2, sqrt(l), J = d xi / d delta_s (= -d xi / d delta_t, left perturbations
//      P <- [exp(omega) | v] P) and the blocks B = l J^T Lambda J, c = l J^T Lambda xi;
//   2. assembly of the dense normal matrix W = H + lambda diag(H) of the 6 (n - 1) unknowns in global memory (L2
//      resident: 4.6 MB at the 128-node cap, beyond LDS from ~22 nodes on): entry (a, b) of the block row of node i is
//      owned by ONE thread, which walks the node's incident edges in ascending edge index (CSR built once per call);
//   3. blocked right-looking Cholesky (panels of PG_NB columns staged in LDS, 4x4 register tiles in the trailing update),
//      forward and back substitution by panels;
//   4. trial poses, trial objective, accept / reject, lambda update.
// Determinism: no atomics; every sum has a fixed order that depends on the graph alone (an edge's terms are summed per
// thread in strided order, per wave by a butterfly, over the four waves in order), and every element of W has one owner
// per phase.  Two runs agree bit for bit and a graph's result does not depend on the other graphs of the call.
#include "dgr_internal.h"

#include <cmath>
#include <cstring>

constexpr int PG_THREADS = 256;
constexpr int PG_MAX_NODES = DGR_PG_MAX_NODES;
constexpr int PG_MAX_M = 6 * (PG_MAX_NODES - 1);   // 762 unknowns
constexpr int PG_NB = 8;                            // Cholesky panel width: a panel of 762 rows is 48 KiB of LDS
constexpr double PG_LAMBDA_INIT = 1e-6, PG_LAMBDA_MIN = 1e-12, PG_LAMBDA_MAX = 1e8, PG_STEP_TOL = 1e-13;

struct PgGraph {
  int64_t node0, edge0;   // first node / edge of the graph in the call's arrays
  int64_t w_off;          // first element of the graph's normal matrix
  int64_t adj0;           // first entry of the graph's adjacency lists (2 per edge)
  int32_t n, ne, ref, max_iter;
  double mu, rel_tol;
};

// ---- small fixed-size helpers ------------------------------------------------------------------------------------
__device__ __forceinline__ void pg_cross_mat(const double *v, double K[9]) {
  K[0] = 0.0; K[1] = -v[2]; K[2] = v[1];
  K[3] = v[2]; K[4] = 0.0; K[5] = -v[0];
  K[6] = -v[1]; K[7] = v[0]; K[8] = 0.0;
}
__device__ __forceinline__ void pg_mul33(const double *A, const double *B, double *C) {   // C = A B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// The rotation vector (axis times angle, angle in [0, pi]) of a rotation matrix: eval.metrics.rotation_vector, with its
// care near 0 (the antisymmetric part IS the vector) and near pi (the axis from the symmetric part).
__device__ void pg_rotation_vector(const double *R, double *w) {
  w[0] = 0.5 * (R[7] - R[5]);
  w[1] = 0.5 * (R[2] - R[6]);
  w[2] = 0.5 * (R[3] - R[1]);
  const double s = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
  const double angle = atan2(s, c);
  if (s > 1e-6) {
    const double f = angle / s;
    w[0] *= f; w[1] *= f; w[2] *= f;
    return;
  }
  if (c > 0.0) return;
  // angle -> pi: (R + R^T) / 2 - c I = (1 - c) a a^T; the row of the largest diagonal entry, normalised.  That row knows
  // the axis up to its sign; the sign is the antisymmetric part's (w = sin(angle) a: tiny here, but far above rounding),
  // and where w is exactly zero the angle is pi and both signs are logarithms.  (2 w is taken from R again: w kept alive
  // over A costs 4 registers more than the 256 at which two waves fit a SIMD.)
  double A[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = 0.5 * (R[3 * i + j] + R[3 * j + i]) - (i == j ? c : 0.0);
  int k = 0;
  if (A[4] > A[0]) k = 1;
  if (A[8] > A[4 * k]) k = 2;
  double a[3] = {A[3 * k], A[3 * k + 1], A[3 * k + 2]};
  const double nrm = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const double f = nrm > 0.0 ? copysign(angle / nrm, a[0] * (R[7] - R[5]) + a[1] * (R[2] - R[6]) + a[2] * (R[3] - R[1])) : 0.0;
  w[0] = a[0] * f; w[1] = a[1] * f; w[2] = a[2] * f;
}

// THE residual: E = inv(P_t) P_s inv(X) as rotation RE [9] and translation tE [3], xi = (rotation vector of E, tE).
// Poses are 12 doubles (row-major 3x4), X a row-major 4x4 whose last row is ignored; all taken as rigid.
__device__ void pg_residual(const double *Ps, const double *Pt, const double *X, double *RE, double *tE, double *xi) {
  double M[9], tM[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) M[3 * i + j] = Pt[i] * Ps[j] + Pt[4 + i] * Ps[4 + j] + Pt[8 + i] * Ps[8 + j];   // R_t^T R_s
    tM[i] = Pt[i] * (Ps[3] - Pt[3]) + Pt[4 + i] * (Ps[7] - Pt[7]) + Pt[8 + i] * (Ps[11] - Pt[11]);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) RE[3 * i + j] = M[3 * i] * X[4 * j] + M[3 * i + 1] * X[4 * j + 1] + M[3 * i + 2] * X[4 * j + 2];
  for (int i = 0; i < 3; ++i) tE[i] = tM[i] - (RE[3 * i] * X[3] + RE[3 * i + 1] * X[7] + RE[3 * i + 2] * X[11]);
  pg_rotation_vector(RE, xi);
  xi[3] = tE[0]; xi[4] = tE[1]; xi[5] = tE[2];
}

__device__ __forceinline__ double pg_quad6(const double *L, const double *x) {   // x^T L x, fixed order
  double q = 0.0;
  for (int a = 0; a < 6; ++a) {
    double r = 0.0;
    for (int b = 0; b < 6; ++b) r += L[6 * a + b] * x[b];
    q += x[a] * r;
  }
  return q;
}

// sum over the block, the same value in every thread; `red` is 4 doubles of LDS (free again on return)
__device__ double pg_block_sum(double v, double *red) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}
__device__ double pg_block_max(double v, double *red) {
  for (int s = 32; s >= 1; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return t;
}

struct PgArrays {
  const PgGraph *graphs;
  const int32_t *edge_ids;    // [E,2] graph-local (s, t)
  const double *edge_T;       // [E,16]
  const double *edge_info;    // [E,36]
  const uint8_t *edge_unc;    // [E]
  const int32_t *adj_ptr;     // per graph n + 1 entries at node0 + graph index
  const int32_t *adj;         // [2E] incident edges of every node, ascending edge index; bit 31 set: the node is the edge's t
  double *pose, *trial;       // [N,12]
  double *eB, *ec;            // [E,36], [E,6]: l J^T Lambda J, l J^T Lambda xi
  double *ew;                 // [E] sqrt(l) of the current outer iteration (1 on certain edges)
  double *W;                  // the graphs' normal matrices back to back
  double *line_out;           // [E]
  double *stats_out;          // [ngraphs,4]
};

// Edge pass over the poses `P`.  FULL: stores sqrt(l), B, c of the linearisation at P and returns the edge's term of F*;
// otherwise returns its term of the frozen-weight objective under the stored sqrt(l).
template <bool FULL>
__device__ double pg_edge_pass(const PgArrays &A, const PgGraph &G, const double *P) {
  double acc = 0.0;
  for (int e = threadIdx.x; e < G.ne; e += PG_THREADS) {
    const int64_t ge = G.edge0 + e;
    const int s = A.edge_ids[2 * ge], t = A.edge_ids[2 * ge + 1];
    const double *Pt = P + (G.node0 + t) * 12;
    const double *L = A.edge_info + ge * 36;
    double RE[9], tE[3], xi[6];
    pg_residual(P + (G.node0 + s) * 12, Pt, A.edge_T + ge * 16, RE, tE, xi);
    const double chi2 = pg_quad6(L, xi);
    const bool unc = A.edge_unc[ge] != 0;
    if (!FULL) {
      const double w = A.ew[ge];
      acc += unc ? w * w * chi2 + G.mu * ((w - 1.0) * (w - 1.0)) : chi2;
      continue;
    }
    const double w = unc ? G.mu / (G.mu + chi2) : 1.0;
    A.ew[ge] = w;
    acc += unc ? G.mu * chi2 / (G.mu + chi2) : chi2;
    // J = [[Jl^-1(omega) R_t^T, 0], [[t' - t_E]x R_t^T, R_t^T]],  t' = -R_t^T t_t
    double Rtt[9], K[9], K2[9], Ji[9], J[36], u[3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Rtt[3 * i + j] = Pt[4 * j + i];
    const double th2 = xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2];
    const double th = sqrt(th2);
    const double cc = th < 1e-3 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - cos(0.5 * th) / (2.0 * th * sin(0.5 * th));
    pg_cross_mat(xi, K);
    pg_mul33(K, K, K2);
    for (int i = 0; i < 9; ++i) Ji[i] = ((i % 4 == 0) ? 1.0 : 0.0) - 0.5 * K[i] + cc * K2[i];
    for (int i = 0; i < 3; ++i) u[i] = -(Rtt[3 * i] * Pt[3] + Rtt[3 * i + 1] * Pt[7] + Rtt[3 * i + 2] * Pt[11]) - tE[i];
    pg_cross_mat(u, K);
    double J11[9], J21[9];
    pg_mul33(Ji, Rtt, J11);
    pg_mul33(K, Rtt, J21);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        J[6 * i + j] = J11[3 * i + j];
        J[6 * i + 3 + j] = 0.0;
        J[6 * (3 + i) + j] = J21[3 * i + j];
        J[6 * (3 + i) + 3 + j] = Rtt[3 * i + j];
      }
    const double l = w * w;
    double Lx[6];
    for (int a = 0; a < 6; ++a) {
      double r = 0.0;
      for (int b = 0; b < 6; ++b) r += L[6 * a + b] * xi[b];
      Lx[a] = r;
    }
    double *B = A.eB + ge * 36, *c = A.ec + ge * 6;
    for (int a = 0; a < 6; ++a) {
      double r = 0.0;
      for (int b = 0; b < 6; ++b) r += J[6 * b + a] * Lx[b];
      c[a] = l * r;
    }
    // B = l J^T (Lambda J), column by column of Lambda J
    for (int b = 0; b < 6; ++b) {
      double LJ[6];
      for (int a = 0; a < 6; ++a) {
        double r = 0.0;
        for (int k = 0; k < 6; ++k) r += L[6 * a + k] * J[6 * k + b];
        LJ[a] = r;
      }
      for (int a = 0; a < 6; ++a) {
        double r = 0.0;
        for (int k = 0; k < 6; ++k) r += J[6 * k + a] * LJ[k];
        B[6 * a + b] = l * r;
      }
    }
  }
  return acc;
}

__device__ __forceinline__ int pg_slot(int node, int ref) { return node < ref ? node : node - 1; }

// W = H + lambda diag(H) (lower triangle, row-major, leading dimension m) and rhs = -g.  Work item = (node, a, b): the
// thread owns row 6 slot + a of the node's block row at column offset b of every block, and walks the node's incident
// edges in ascending edge index.
__device__ void pg_assemble(const PgArrays &A, const PgGraph &G, double *W, int m, double lambda, double *rhs) {
  for (int i = 0; i < m; ++i)   // the lower triangle only: nothing reads the rest
    for (int j = threadIdx.x; j <= i; j += PG_THREADS) W[(int64_t)i * m + j] = 0.0;
  __syncthreads();
  const int32_t *ptr = A.adj_ptr + G.node0 + blockIdx.x;   // (n + 1 entries per graph)
  const int32_t *adj = A.adj + G.adj0;
  for (int item = threadIdx.x; item < G.n * 36; item += PG_THREADS) {
    const int node = item / 36, a = (item % 36) / 6, b = item % 6;
    if (node == G.ref) continue;
    const int row = 6 * pg_slot(node, G.ref) + a;
    double diag = 0.0, g = 0.0;
    for (int32_t k = ptr[node]; k < ptr[node + 1]; ++k) {
      const int32_t rec = adj[k];
      const int e = rec & 0x7fffffff;
      const bool is_t = rec < 0;
      const int64_t ge = G.edge0 + e;
      const double v = A.eB[ge * 36 + 6 * a + b];
      diag += v;
      if (b == 0) g += is_t ? -A.ec[ge * 6 + a] : A.ec[ge * 6 + a];
      const int other = A.edge_ids[2 * ge + (is_t ? 0 : 1)];
      if (other == G.ref) continue;
      const int oslot = pg_slot(other, G.ref);
      if (6 * oslot < 6 * pg_slot(node, G.ref))   // the lower triangle: blocks left of the diagonal block
        W[(int64_t)row * m + 6 * oslot + b] -= v;
    }
    if (b <= a) W[(int64_t)row * m + (row - a) + b] = (a == b) ? diag + lambda * (diag > 0.0 ? diag : 1.0) : diag;
    if (b == 0) rhs[row] = -g;
  }
  __syncthreads();
}

// In-place Cholesky of the lower triangle of W (m x m).  Returns false (in every thread) at a pivot that is not
// positive.  `pan` holds rows [k0, m) of the current panel: pan[(i - k0) * PG_NB + c].
__device__ bool pg_cholesky(double *W, int m, double *pan) {
  for (int k0 = 0; k0 < m; k0 += PG_NB) {
    const int nb = min(PG_NB, m - k0), k1 = k0 + nb;
    for (int i = k0 + threadIdx.x; i < m; i += PG_THREADS)
      for (int c = 0; c < PG_NB; ++c) pan[(i - k0) * PG_NB + c] = (c < nb && k0 + c <= i) ? W[(int64_t)i * m + k0 + c] : 0.0;
    __syncthreads();
    // the diagonal block, factored by every thread for itself (the same arithmetic on the same values: no exchange)
    double D[PG_NB][PG_NB];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < PG_NB; ++c) {
#pragma unroll
      for (int r = 0; r < PG_NB; ++r) D[r][c] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < PG_NB; ++c) {
      if (c < nb) {
        double d = pan[c * PG_NB + c];
#pragma unroll
        for (int k = 0; k < c; ++k) d -= D[c][k] * D[c][k];
        if (!(d > 0.0) || !(d < INFINITY)) ok = false;
        d = ok ? sqrt(d) : 1.0;
        D[c][c] = d;
#pragma unroll
        for (int r = c + 1; r < PG_NB; ++r) {
          if (r < nb) {
            double v = pan[r * PG_NB + c];
#pragma unroll
            for (int k = 0; k < c; ++k) v -= D[r][k] * D[c][k];
            D[r][c] = v / d;
          }
        }
      }
    }
    if (!ok) return false;   // (uniform: every thread computed the same block)
    if (threadIdx.x < nb * PG_NB) {
      const int r = threadIdx.x / PG_NB, c = threadIdx.x % PG_NB;
      if (c <= r && c < nb) {
        double v = 0.0;
#pragma unroll
        for (int rr = 0; rr < PG_NB; ++rr)
#pragma unroll
          for (int cc = 0; cc < PG_NB; ++cc)
            if (rr == r && cc == c) v = D[rr][cc];
        W[(int64_t)(k0 + r) * m + k0 + c] = v;
      }
    }
    // the rows below: x D^T = a, one row per thread
    for (int i = k1 + threadIdx.x; i < m; i += PG_THREADS) {
      double x[PG_NB];
      double *row = pan + (i - k0) * PG_NB;
#pragma unroll
      for (int c = 0; c < PG_NB; ++c) {
        double v = row[c];
#pragma unroll
        for (int k = 0; k < c; ++k) v -= x[k] * D[c][k];
        x[c] = (c < nb) ? v / D[c][c] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < PG_NB; ++c) {
        row[c] = x[c];
        if (c < nb) W[(int64_t)i * m + k0 + c] = x[c];
      }
    }
    __syncthreads();
    // trailing update of the lower triangle of rows / columns [k1, m): 4x4 tiles, tile t = (bi, bj), bj <= bi
    const int r = m - k1, nt = (r + 3) / 4, tiles = nt * (nt + 1) / 2;
    for (int t = threadIdx.x; t < tiles; t += PG_THREADS) {
      int bi = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
      while (bi * (bi + 1) / 2 > t) --bi;
      const int bj = t - bi * (bi + 1) / 2;
      const int i0 = k1 + 4 * bi, j0 = k1 + 4 * bj;
      double acc[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
#pragma unroll
      for (int c = 0; c < PG_NB; ++c) {
        double li[4], lj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          li[a] = (i0 + a < m) ? pan[(i0 + a - k0) * PG_NB + c] : 0.0;
          lj[a] = (j0 + a < m) ? pan[(j0 + a - k0) * PG_NB + c] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] += li[a] * lj[b];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = i0 + a, j = j0 + b;
          if (i < m && j <= i) W[(int64_t)i * m + j] -= acc[a][b];
        }
    }
    __syncthreads();
  }
  return true;
}

// L L^T x = rhs by panels; x ends in `rhs`, `sol` is the intermediate (both m doubles of LDS)
__device__ void pg_solve(const double *W, int m, double *rhs, double *sol) {
  for (int k0 = 0; k0 < m; k0 += PG_NB) {   // L y = rhs: y -> sol
    const int nb = min(PG_NB, m - k0), k1 = k0 + nb;
    double y[PG_NB];
#pragma unroll
    for (int c = 0; c < PG_NB; ++c) {
      y[c] = 0.0;
      if (c < nb) {
        double v = rhs[k0 + c];
#pragma unroll
        for (int k = 0; k < c; ++k) v -= W[(int64_t)(k0 + c) * m + k0 + k] * y[k];
        y[c] = v / W[(int64_t)(k0 + c) * m + k0 + c];
      }
    }
    if (threadIdx.x < nb) {
      double v = 0.0;
#pragma unroll
      for (int c = 0; c < PG_NB; ++c)
        if (c == (int)threadIdx.x) v = y[c];
      sol[k0 + threadIdx.x] = v;
    }
    for (int i = k1 + threadIdx.x; i < m; i += PG_THREADS) {
      double v = rhs[i];
#pragma unroll
      for (int c = 0; c < PG_NB; ++c)
        if (c < nb) v -= W[(int64_t)i * m + k0 + c] * y[c];
      rhs[i] = v;
    }
    __syncthreads();
  }
  const int last = ((m - 1) / PG_NB) * PG_NB;
  for (int k0 = last; k0 >= 0; k0 -= PG_NB) {   // L^T x = sol: x -> rhs
    const int nb = min(PG_NB, m - k0);
    double x[PG_NB];
#pragma unroll
    for (int c = PG_NB - 1; c >= 0; --c) {
      x[c] = 0.0;
      if (c < nb) {
        double v = sol[k0 + c];
#pragma unroll
        for (int k = PG_NB - 1; k > c; --k)
          if (k < nb) v -= W[(int64_t)(k0 + k) * m + k0 + c] * x[k];
        x[c] = v / W[(int64_t)(k0 + c) * m + k0 + c];
      }
    }
    if (threadIdx.x < nb) {
      double v = 0.0;
#pragma unroll
      for (int c = 0; c < PG_NB; ++c)
        if (c == (int)threadIdx.x) v = x[c];
      rhs[k0 + threadIdx.x] = v;
    }
    for (int j = threadIdx.x; j < k0; j += PG_THREADS) {
      double v = sol[j];
#pragma unroll
      for (int c = 0; c < PG_NB; ++c)
        if (c < nb) v -= W[(int64_t)(k0 + c) * m + j] * x[c];
      sol[j] = v;
    }
    __syncthreads();
  }
}

// trial = [exp([omega]x) | v] . pose per node (the reference node: copied); returns the largest |delta| entry seen by
// this thread
__device__ double pg_retract(const PgGraph &G, const double *delta, const double *pose, double *trial) {
  double big = 0.0;
  for (int node = threadIdx.x; node < G.n; node += PG_THREADS) {
    const double *P = pose + (G.node0 + node) * 12;
    double *Q = trial + (G.node0 + node) * 12;
    if (node == G.ref) {
      for (int k = 0; k < 12; ++k) Q[k] = P[k];
      continue;
    }
    const double *d = delta + 6 * pg_slot(node, G.ref);
    for (int k = 0; k < 6; ++k) big = fmax(big, fabs(d[k]));
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double th = sqrt(th2);
    const double a = th < 1e-4 ? 1.0 - th2 / 6.0 : sin(th) / th;
    const double b = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
    double K[9], K2[9], R[9];
    pg_cross_mat(d, K);
    pg_mul33(K, K, K2);
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * K[i] + b * K2[i];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 4; ++j) Q[4 * i + j] = R[3 * i] * P[j] + R[3 * i + 1] * P[4 + j] + R[3 * i + 2] * P[8 + j];
      Q[4 * i + 3] += d[3 + i];
    }
  }
  return big;
}

__global__ void __launch_bounds__(PG_THREADS) pg_optimize_kernel(PgArrays A) {
  __shared__ double pan[PG_MAX_M * PG_NB];
  __shared__ double rhs[PG_MAX_M + 6], sol[PG_MAX_M + 6];
  __shared__ double red[4];
  const PgGraph &G = A.graphs[blockIdx.x];
  const int m = 6 * (G.n - 1);
  double *W = A.W + G.w_off;
  double *pose = A.pose, *trial = A.trial;

  double F = pg_block_sum(pg_edge_pass<true>(A, G, pose), red);
  const double F0 = F;
  double lambda = PG_LAMBDA_INIT;
  int iterations = 0, converged = 0;
#ifdef DGR_PG_TIMING   // build with EXTRA=-DDGR_PG_TIMING: thread 0 prints where the loop's time went (tools/pose_graph_bench.py)
  long long tk[4] = {0, 0, 0, 0}, t0 = wall_clock64(), t1;
  const long long t_begin = t0;
  int nfact = 0;
#define PG_TICK(i) do { t1 = wall_clock64(); tk[i] += t1 - t0; t0 = t1; } while (0)
#else
#define PG_TICK(i) do { } while (0)
#endif
  for (int it = 0; it < G.max_iter && m > 0; ++it) {
    bool accepted = false;
    double step = 0.0;
    for (;;) {
      PG_TICK(3);
      pg_assemble(A, G, W, m, lambda, rhs);
      PG_TICK(0);
      bool ok = pg_cholesky(W, m, pan);
      __syncthreads();
      PG_TICK(1);
#ifdef DGR_PG_TIMING
      ++nfact;
#endif
      if (ok) {
        pg_solve(W, m, rhs, sol);
        PG_TICK(2);
        step = pg_block_max(pg_retract(G, rhs, pose, trial), red);
        __syncthreads();
        const double Ft = pg_block_sum(pg_edge_pass<false>(A, G, trial), red);
        if (step < INFINITY && Ft <= F) {   // (a NaN anywhere fails both tests)
          accepted = true;
          break;
        }
      }
      lambda *= 10.0;
      if (lambda > PG_LAMBDA_MAX) break;
    }
    if (!accepted) {   // no descent left at any damping: the numerical floor
      converged = 1;
      break;
    }
    double *tmp = pose; pose = trial; trial = tmp;
    const double Fn = pg_block_sum(pg_edge_pass<true>(A, G, pose), red);
    const double dec = F - Fn, Fold = F;
    F = Fn;
    ++iterations;
    lambda = fmax(lambda * 0.1, PG_LAMBDA_MIN);
    if (dec <= G.rel_tol * Fold || step <= PG_STEP_TOL) {
      converged = 1;
      break;
    }
  }
  if (m == 0) converged = 1;
  // the result goes to A.pose whichever buffer holds it; the line processes of the final poses
  __syncthreads();
  if (pose != A.pose)
    for (int i = threadIdx.x; i < G.n * 12; i += PG_THREADS) A.pose[G.node0 * 12 + i] = pose[G.node0 * 12 + i];
  for (int e = threadIdx.x; e < G.ne; e += PG_THREADS) {
    const double w = A.ew[G.edge0 + e];
    A.line_out[G.edge0 + e] = w * w;
  }
#ifdef DGR_PG_TIMING
  PG_TICK(3);
  if (threadIdx.x == 0)   // wall_clock64 ticks at 100 MHz
    printf("pg timing: graph %d n %d edges %d steps %d factorisations %d total_us %.1f assemble_us %.1f cholesky_us %.1f "
           "solve_us %.1f edges_us %.1f\n", (int)blockIdx.x, G.n, G.ne, iterations, nfact, (t0 - t_begin) * 0.01, tk[0] * 0.01,
           tk[1] * 0.01, tk[2] * 0.01, tk[3] * 0.01);
#endif
  if (threadIdx.x == 0) {
    double *s = A.stats_out + 4 * (int64_t)blockIdx.x;
    s[0] = F0; s[1] = F; s[2] = (double)iterations; s[3] = (double)converged;
  }
}

static bool pg_finite(const double *v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

extern "C" int dgr_pose_graph_optimize(dgr_ctx *ctx, int ngraphs, const int64_t *node_off, const int64_t *edge_off,
                                       const int32_t *edge_ids, const double *edge_T, const double *edge_info,
                                       const uint8_t *edge_uncertain, const double *pose_init, const dgr_pg_params *params,
                                       double *pose_out, double *line_out, double *stats_out, dgr_stream stream_) {
  // argument errors first: nothing has touched the device when one of them is reported
  DGR_REQUIRE(ctx && node_off && edge_off && edge_ids && edge_T && edge_info && edge_uncertain && pose_init && params &&
                  pose_out && line_out && stats_out,
              "dgr_pose_graph_optimize: NULL argument");
  DGR_REQUIRE(ngraphs >= 1 && ngraphs <= 65535, "dgr_pose_graph_optimize: ngraphs = %d (1..65535)", ngraphs);
  DGR_REQUIRE(node_off[0] == 0 && edge_off[0] == 0, "dgr_pose_graph_optimize: offsets must start at 0");
  std::vector<PgGraph> hg(ngraphs);
  int64_t w_total = 0;
  for (int g = 0; g < ngraphs; ++g) {
    const int64_t n = node_off[g + 1] - node_off[g], ne = edge_off[g + 1] - edge_off[g];
    DGR_REQUIRE(n >= 1 && ne >= 1, "dgr_pose_graph_optimize: graph %d is empty (%lld nodes, %lld edges)", g, (long long)n,
                (long long)ne);
    DGR_REQUIRE(n <= PG_MAX_NODES, "dgr_pose_graph_optimize: graph %d has %lld nodes (at most %d)", g, (long long)n,
                PG_MAX_NODES);
    DGR_REQUIRE(ne < (1 << 24), "dgr_pose_graph_optimize: graph %d has %lld edges", g, (long long)ne);
    const dgr_pg_params &p = params[g];
    DGR_REQUIRE(p.mu > 0.0 && std::isfinite(p.mu), "dgr_pose_graph_optimize: graph %d: mu must be positive and finite", g);
    DGR_REQUIRE(p.reference_node >= 0 && p.reference_node < n, "dgr_pose_graph_optimize: graph %d: reference node %d outside [0, %lld)",
                g, p.reference_node, (long long)n);
    DGR_REQUIRE(p.max_iter >= 0 && p.max_iter <= 100000, "dgr_pose_graph_optimize: graph %d: max_iter = %d", g, p.max_iter);
    DGR_REQUIRE(p.rel_tol >= 0.0 && std::isfinite(p.rel_tol), "dgr_pose_graph_optimize: graph %d: rel_tol must be >= 0 and finite", g);
    for (int64_t e = edge_off[g]; e < edge_off[g + 1]; ++e) {
      const int32_t s = edge_ids[2 * e], t = edge_ids[2 * e + 1];
      DGR_REQUIRE(s >= 0 && s < n && t >= 0 && t < n, "dgr_pose_graph_optimize: graph %d: edge (%d, %d) outside [0, %lld)", g, s, t,
                  (long long)n);
      DGR_REQUIRE(s != t, "dgr_pose_graph_optimize: graph %d: edge from node %d to itself", g, s);
      DGR_REQUIRE(pg_finite(edge_T + e * 16, 12), "dgr_pose_graph_optimize: graph %d: non-finite edge pose", g);
      DGR_REQUIRE(pg_finite(edge_info + e * 36, 36), "dgr_pose_graph_optimize: graph %d: non-finite information matrix", g);
    }
    for (int64_t i = node_off[g]; i < node_off[g + 1]; ++i)
      DGR_REQUIRE(pg_finite(pose_init + i * 16, 12), "dgr_pose_graph_optimize: graph %d: non-finite initial pose", g);
    PgGraph &G = hg[g];
    memset(&G, 0, sizeof(G));
    G.node0 = node_off[g]; G.edge0 = edge_off[g];
    G.n = (int32_t)n; G.ne = (int32_t)ne;
    G.ref = p.reference_node; G.max_iter = p.max_iter;
    G.mu = p.mu; G.rel_tol = p.rel_tol;
    G.adj0 = 2 * edge_off[g];
    G.w_off = w_total;
    w_total += (int64_t)(6 * (n - 1)) * (6 * (n - 1));
  }
  const int64_t N = node_off[ngraphs], E = edge_off[ngraphs];

  // one staging buffer: graphs | adjacency pointers | adjacency | edge ids | flags | edge poses | information | poses
  std::vector<int32_t> adj_ptr(N + ngraphs), adj(2 * E);
  for (int g = 0; g < ngraphs; ++g) {
    const PgGraph &G = hg[g];
    int32_t *ptr = adj_ptr.data() + G.node0 + g;
    std::vector<int32_t> deg(G.n + 1, 0);
    for (int e = 0; e < G.ne; ++e) {
      ++deg[edge_ids[2 * (G.edge0 + e)]];
      ++deg[edge_ids[2 * (G.edge0 + e) + 1]];
    }
    ptr[0] = 0;
    for (int i = 0; i < G.n; ++i) ptr[i + 1] = ptr[i] + deg[i];
    std::vector<int32_t> fill(ptr, ptr + G.n);
    for (int e = 0; e < G.ne; ++e) {   // ascending edge index within every node's list
      adj[G.adj0 + fill[edge_ids[2 * (G.edge0 + e)]]++] = e;
      adj[G.adj0 + fill[edge_ids[2 * (G.edge0 + e) + 1]]++] = (int32_t)((uint32_t)e | 0x80000000u);
    }
  }
  std::vector<double> pose12((size_t)N * 12);
  for (int64_t i = 0; i < N; ++i) memcpy(&pose12[i * 12], pose_init + i * 16, 12 * sizeof(double));

  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &Ar = ctx->arena;
  const size_t out_doubles = (size_t)N * 12 + (size_t)E + (size_t)ngraphs * 4;
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64 + out_doubles * sizeof(double), &pin));
  PgGraph *d_graphs;
  int32_t *d_adj_ptr, *d_adj, *d_ids;
  uint8_t *d_unc;
  double *d_T, *d_info, *d_out;
  PgArrays A;
  DGR_ALLOC(d_graphs, Ar, PgGraph, ngraphs);
  DGR_ALLOC(d_adj_ptr, Ar, int32_t, N + ngraphs);
  DGR_ALLOC(d_adj, Ar, int32_t, 2 * E);
  DGR_ALLOC(d_ids, Ar, int32_t, 2 * E);
  DGR_ALLOC(d_unc, Ar, uint8_t, E);
  DGR_ALLOC(d_T, Ar, double, E * 16);
  DGR_ALLOC(d_info, Ar, double, E * 36);
  DGR_ALLOC(d_out, Ar, double, out_doubles);   // poses [N,12] | line processes [E] | stats [ngraphs,4]
  DGR_ALLOC(A.trial, Ar, double, N * 12);
  DGR_ALLOC(A.eB, Ar, double, E * 36);
  DGR_ALLOC(A.ec, Ar, double, E * 6);
  DGR_ALLOC(A.ew, Ar, double, E);
  DGR_ALLOC(A.W, Ar, double, w_total);
  A.graphs = d_graphs; A.edge_ids = d_ids; A.edge_T = d_T; A.edge_info = d_info; A.edge_unc = d_unc;
  A.adj_ptr = d_adj_ptr; A.adj = d_adj;
  A.pose = d_out; A.line_out = d_out + N * 12; A.stats_out = d_out + N * 12 + E;
  // the host arrays are read by asynchronous copies: they live until this function returns, and it does not return
  // before the stream is idle
  DGR_HIP_CHECK(hipMemcpyAsync(d_graphs, hg.data(), (size_t)ngraphs * sizeof(PgGraph), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(d_adj_ptr, adj_ptr.data(), adj_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(d_adj, adj.data(), adj.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(d_ids, edge_ids, (size_t)E * 2 * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(d_unc, edge_uncertain, (size_t)E, hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(d_T, edge_T, (size_t)E * 16 * sizeof(double), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(d_info, edge_info, (size_t)E * 36 * sizeof(double), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(A.pose, pose12.data(), pose12.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  pg_optimize_kernel<<<ngraphs, PG_THREADS, 0, stream>>>(A);
  DGR_LAUNCH_CHECK();
  DGR_HIP_CHECK(hipMemcpyAsync(pin + 64, d_out, out_doubles * sizeof(double), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // the call's one synchronisation
  const double *res = reinterpret_cast<const double *>(pin + 64);
  for (int64_t i = 0; i < N; ++i) {
    // the gauge node and the last rows are the caller's own values, bit for bit
    memcpy(pose_out + i * 16, pose_init + i * 16, 16 * sizeof(double));
    memcpy(pose_out + i * 16, res + i * 12, 12 * sizeof(double));
  }
  for (int g = 0; g < ngraphs; ++g) {
    const int64_t r = node_off[g] + params[g].reference_node;
    memcpy(pose_out + r * 16, pose_init + r * 16, 16 * sizeof(double));
  }
  memcpy(line_out, res + N * 12, (size_t)E * sizeof(double));
  memcpy(stats_out, res + N * 12 + E, (size_t)ngraphs * 4 * sizeof(double));
  return DGR_OK;
}
