// gmm_px_prep.hip -- the EM loop's whitening of a plain GMM p(x) on the device: Cholesky, triangular inverse and the packing
// of the log-density operands, one workgroup per mixture (gmm_px_prepare_device, declared in gmmmap_handle.hpp; called by
// estep_full.hip and gmm_em.hip).
#include "vcmi_common.hpp"
#include "gmmmap_handle.hpp"
#include "hostpipe.hpp"

#include <cmath>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// p(x) preparation on the device (used by the EM loop: the parameters never leave HBM between iterations).
// One workgroup per mixture: Hermitian(Sigma) (upper triangle mirrored, src/gmm.jl:16) -> right-looking Cholesky in
// LDS -> U = L^-1 by forward substitution (thread = column) -> cz = U mu, lc = log w - (D log 2pi + logdet)/2 ->
// row-major U/cz/lc for the generic kernels and the U-only MFMA operand blocks in issue order.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
px_prep_kernel(const double *__restrict__ w, const double *__restrict__ mu, const double *__restrict__ sigma, int D, int DP,
               const int *__restrict__ table, int nsteps, int cinit_off, int ncinit, int lc_off, int blk_len,
               double *__restrict__ U, double *__restrict__ cz, double *__restrict__ lc, double *__restrict__ packedU,
               int *__restrict__ flag) {
  extern __shared__ double smem_px[];
  const int LD = D + 1, tid = threadIdx.x, m = blockIdx.x;
  double *S = smem_px;                    // [D][LD] covariance, then its lower Cholesky factor
  double *V = S + (size_t)D * LD;         // [D][LD] U = L^-1 (lower)
  __shared__ double czs[256];
  __shared__ double lcs;
  __shared__ int bad;
  const double *Sg = sigma + (size_t)m * D * D;
  for (int e = tid; e < D * D; e += 256) {
    const int r = e / D, c = e - r * D;
    S[r * LD + c] = (r <= c) ? Sg[r + (size_t)D * c] : Sg[c + (size_t)D * r];
    V[r * LD + c] = (r == c) ? 1.0 : 0.0;
  }
  if (tid == 0) bad = 0;
  __syncthreads();
  // Cholesky and U = L^-1 in ONE loop over the columns: the row operations that eliminate column j of L (row j scaled by
  // 1 / l_jj, row i -= l_ij row j) are applied to the identity beside it -- row j of V is final when its step comes, and the
  // updates of a step are independent of each other (threads as a 16 x 16 grid over (row, column)).  Round 5: the inverse used
  // to be a forward substitution AFTER the loop, one thread per column walking 3200 dependent multiply-adds through LDS:
  // two thirds of this kernel's 181 us.
  for (int j = 0; j < D; ++j) {
    const double d = S[j * LD + j];
    if (!(d > 0.0) && tid == 0) bad = 1;
    const double sd = sqrt(d), isd = 1.0 / sd;
    __syncthreads();                      // every thread has read the pivot
    for (int i = j + tid; i < D; i += 256) S[i * LD + j] = (i == j) ? sd : S[i * LD + j] / sd;
    for (int c = tid; c <= j; c += 256) V[j * LD + c] *= isd;
    __syncthreads();
    for (int i = j + 1 + (tid >> 4); i < D; i += 16) {
      const double lij = S[i * LD + j];
      // trailing update of the lower triangle: no division per element
      for (int k = j + 1 + (tid & 15); k <= i; k += 16) S[i * LD + k] = fma(-lij, S[k * LD + j], S[i * LD + k]);
      // the same row operation on the identity's rows: columns 0 .. j of row i
      for (int c = (tid & 15); c <= j; c += 16) V[i * LD + c] = fma(-lij, V[j * LD + c], V[i * LD + c]);
    }
    // (all operands first, then the products, then the stores -- 7 x 7 guarded elements per thread, unrolled -- was tried
    // against the dependent read-modify-writes of these loops: 435 us instead of 145, most of its slots are empty at D = 80)
    __syncthreads();
  }
  if (tid < D) {
    double s = 0.0;
    for (int c = 0; c <= tid; ++c) s = fma(V[tid * LD + c], mu[c + (size_t)D * m], s);
    czs[tid] = s;
  } else if (tid == 255) {
    double ld = 0.0;
    for (int d = 0; d < D; ++d) ld += log(S[d * LD + d]);
    const double LOG2PI = 1.8378770664093454835606594728112;
    lcs = (w[m] > 0.0) ? log(w[m]) - 0.5 * (D * LOG2PI + 2.0 * ld) : -INFINITY;   // zero weight: posterior 0
  }
  __syncthreads();
  for (int e = tid; e < DP * DP; e += 256) {
    const int r = e / DP, c = e - r * DP;
    U[(size_t)m * DP * DP + e] = (r < D && c <= r) ? V[r * LD + c] : 0.0;
  }
  for (int e = tid; e < DP; e += 256) cz[(size_t)m * DP + e] = (e < D) ? czs[e] : 0.0;
  if (tid == 0) {
    lc[m] = lcs;
    if (bad) atomicMax(flag, m + 1);
  }
  if (packedU) {
    double *blk = packedU + (size_t)m * blk_len;
    for (int e = tid; e < blk_len; e += 256) {
      double v = 0.0;
      const int s = e >> 6, l = e & 63;
      if (s < nsteps) {
        const int t = table[s] >> 16, ks = table[s] & 0xffff;
        const int p = 16 * t + (l & 15), k = 4 * ks + (l >> 4);
        if (p < D && k <= p) v = V[p * LD + k];
      } else if (e >= cinit_off && e < cinit_off + ncinit) {
        const int p = e - cinit_off;
        if (p < D) v = -czs[p];
      } else if (e == lc_off) {
        v = lcs;
      }
      blk[e] = v;
    }
  }
}

// The same preparation for dimensions whose two D x (D+1) images do not fit LDS (99 < D <= 198, e.g. the 160-dimensional joint
// model of delta features): ONE lower triangle in packed storage (D(D+1)/2 doubles: 103 KB at D = 160) holds the
// covariance, then its Cholesky factor, then -- inverted in place, column by column from the last, with the column
// being replaced kept in a D-vector -- U = L^-1.  Outputs: the generic layout only (U, cz, lc: what
// logdens_tiled_kernel reads).
__global__ void __launch_bounds__(512)
px_prep_packed_kernel(const double *__restrict__ w, const double *__restrict__ mu, const double *__restrict__ sigma, int D,
                      int DP, double *__restrict__ U, double *__restrict__ cz, double *__restrict__ lc,
                      int *__restrict__ flag) {
  extern __shared__ double smem_pp[];
  const int tid = threadIdx.x, m = blockIdx.x, NTH = 512;
  double *P = smem_pp;                                   // packed lower triangle: (i, j <= i) at i (i + 1) / 2 + j
  double *col = P + (size_t)D * (D + 1) / 2;             // [D] the column being replaced (inverse), then cz
  __shared__ double lcs;
  __shared__ int bad;
  auto at = [](int i, int j) { return i * (i + 1) / 2 + j; };
  const double *Sg = sigma + (size_t)m * D * D;
  // Hermitian(Sigma): the upper triangle of the column-major block is the matrix (src/gmm.jl:16): (i, j <= i) = Sg(j, i)
  for (int e = tid; e < D * D; e += NTH) {
    const int i = e / D, j = e - i * D;
    if (j <= i) P[at(i, j)] = Sg[j + (size_t)D * i];
  }
  if (tid == 0) bad = 0;
  __syncthreads();
  // right-looking Cholesky
  for (int j = 0; j < D; ++j) {
    const double d = P[at(j, j)];
    if (!(d > 0.0) && tid == 0) bad = 1;
    const double sd = sqrt(d);
    __syncthreads();                                     // every thread has read the pivot
    for (int i = j + tid; i < D; i += NTH) P[at(i, j)] = (i == j) ? sd : P[at(i, j)] / sd;
    __syncthreads();
    const int n = D - 1 - j;
    for (int e = tid; e < n * n; e += NTH) {
      const int ii = e / n, kk = e - ii * n;
      const int i = j + 1 + ii, k = j + 1 + kk;
      if (i >= k) P[at(i, k)] = fma(-P[at(i, j)], P[at(k, j)], P[at(i, k)]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    double ld = 0.0;
    for (int d = 0; d < D; ++d) ld += log(P[at(d, d)]);
    const double LOG2PI = 1.8378770664093454835606594728112;
    lcs = (w[m] > 0.0) ? log(w[m]) - 0.5 * (D * LOG2PI + 2.0 * ld) : -INFINITY;   // zero weight: posterior 0
  }
  // U = L^-1 in place: column j from the columns to its right (already inverse) and the original column j of L:
  //   U_jj = 1 / L_jj,   U_ij = -(sum_{k=j+1..i} U_ik L_kj) U_jj   (i > j)
  for (int j = D - 1; j >= 0; --j) {
    for (int i = j + tid; i < D; i += NTH) col[i] = P[at(i, j)];
    __syncthreads();
    const double ujj = 1.0 / col[j];
    for (int i = j + tid; i < D; i += NTH) {
      double v = ujj;
      if (i > j) {
        double sacc = 0.0;
        for (int k = j + 1; k <= i; ++k) sacc = fma(P[at(i, k)], col[k], sacc);
        v = -sacc * ujj;
      }
      P[at(i, j)] = v;
    }
    __syncthreads();
  }
  // cz = U mu
  for (int i = tid; i < D; i += NTH) {
    double sacc = 0.0;
    for (int c = 0; c <= i; ++c) sacc = fma(P[at(i, c)], mu[c + (size_t)D * m], sacc);
    col[i] = sacc;
  }
  __syncthreads();
  for (int e = tid; e < DP * DP; e += NTH) {
    const int r = e / DP, c = e - r * DP;
    U[(size_t)m * DP * DP + e] = (r < D && c <= r) ? P[at(r, c)] : 0.0;
  }
  for (int e = tid; e < DP; e += NTH) cz[(size_t)m * DP + e] = (e < D) ? col[e] : 0.0;
  if (tid == 0) {
    lc[m] = lcs;
    if (bad) atomicMax(flag, m + 1);
  }
}

static bool px_prep_fits_full(int D) {      // px_prep_kernel: two D x (D+1) images (D <= 99: 158,400 B + 2 KB static of 160 KB)
  return (size_t)2 * D * (D + 1) * sizeof(double) + 4096 <= (size_t)160 * 1024;
}
bool gmm_px_device_prepare_supported(int D) {
  if (D < 1 || D > 256) return false;
  if (px_prep_fits_full(D)) return true;
  // packed variant: only for dimensions whose log-densities do not need the MFMA operand blocks (logdens_tiled_kernel)
  const int DP = (D + 3) / 4 * 4;
  return !gmmmap_has_mfma(DP) && ((size_t)D * (D + 1) / 2 + D) * sizeof(double) + 4096 <= (size_t)160 * 1024;
}

int gmm_px_prepare_device(vcmi_gmmmap **inout, const double *d_w, const double *d_mu, const double *d_sigma, int D, int M,
                          int *d_flag, hipStream_t st) {
  VCMI_TRY(check_device());
  if (!gmm_px_device_prepare_supported(D)) return fail(VCMI_ERR_ARG, "on-device p(x) preparation: dimension %d too large", D);
  VCMI_TRY(gmm_px_handle_here(inout));
  vcmi_gmmmap *g = *inout;
  const int DP = (D + 3) / 4 * 4;
  g->D = D;
  g->DP = DP;
  g->M = M;
  VCMI_TRY(g->U.reserve((size_t)M * DP * DP));
  VCMI_TRY(g->cz.reserve((size_t)M * DP));
  VCMI_TRY(g->lc.reserve((size_t)M));
  const bool mfma = gmmmap_has_mfma(DP);
  TilingRT tl(DP, true);
  if (mfma) {
    VCMI_TRY(g->packedU.reserve((size_t)tl.BLK * M));
    if (g->px_table_dp != DP) {           // the issue order of the U-only blocks (what pack_tiles(1) writes on the host)
      std::vector<int> tab;
      for_each_fragment(tl, 1, [&](int t, int ks) { tab.push_back((t << 16) | ks); });
      VCMI_TRY(upload_now(g->px_table, tab));
      g->px_table_dp = DP;
    }
  }
  if (!px_prep_fits_full(D)) {
    const size_t shp = ((size_t)D * (D + 1) / 2 + D) * sizeof(double);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(px_prep_packed_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)shp));
    hipLaunchKernelGGL(px_prep_packed_kernel, dim3(M), dim3(512), shp, st, d_w, d_mu, d_sigma, D, DP, g->U.p, g->cz.p, g->lc.p,
                       d_flag);
    VCMI_HIP(hipGetLastError());
    return VCMI_OK;
  }
  const size_t shmem = (size_t)2 * D * (D + 1) * sizeof(double);
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(px_prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)shmem));
  hipLaunchKernelGGL(px_prep_kernel, dim3(M), dim3(256), shmem, st, d_w, d_mu, d_sigma, D, DP, mfma ? g->px_table.p : nullptr,
                     mfma ? tl.NSTEPS : 0, tl.CINIT_OFF, tl.NT * 16, tl.LC_OFF, tl.BLK, g->U.p, g->cz.p, g->lc.p,
                     mfma ? g->packedU.p : nullptr, d_flag);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

}  // namespace vcmi
