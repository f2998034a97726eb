// Probe: the left-looking P-symmetric LU (nlu_ldiag_kernel / nlu_lcol_kernel,
// qp_nopiv.hip compiled in) on a synthetic batch of SPD problems read straight
// from their Q (n = Np, no kept rows): µs per launch of every block column,
// and with -DLDIAG_STAMPS the diagonal kernel's phases (thread 0's s_memtime
// at LD_MARK k, averaged over the workgroups of each launch).
//   hipcc --offload-arch=gfx950 -O3 -DLDIAG_STAMPS tools/probe/ldiag_probe.hip -o ldiag
//   ./ldiag B NP
// With -DLDIAG_PLACE every wave of the first diagonal launch also records its
// hardware-id, LDS-allocation and XCC-id registers and its role (raw values
// of a few workgroups are printed, so the field layout can be checked), and
// the probe prints, per elimination phase q, how many CUs have their
// role == q waves on 1, 2, 3 or 4 distinct SIMDs.  A third argument selects
// the role: 0 the rotation (wave + blockIdx.x) & 3 the product used until
// this probe showed it idle, 1 the placement-derived (SIMD id + LDS slot) & 3
// — probe only: it has no fallback for a workgroup whose waves share a SIMD
// (such workgroups are counted and reported) —, 2 the wave index itself.
//   ./ldiag B NP [0|1|2]
#include <hip/hip_runtime.h>
#ifdef LDIAG_PLACE
__device__ unsigned probe_role_cfg[2];   // [0] role mode, [1] LDS-base units per workgroup allocation
__device__ __forceinline__ int probe_role(int w) {
  if (!probe_role_cfg[0]) return (w + (int)(blockIdx.x & 3)) & 3;
  if (probe_role_cfg[0] == 2) return w;
  unsigned hw, la;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_LDS_ALLOC)" : "=s"(la));
  return (int)((((hw >> 4) & 3) + (la & 0xfff) / probe_role_cfg[1]) & 3);
}
#define NLU_ROLE(w) probe_role(w)
#endif
#include "../../diffopt.jl_amd/csrc/qp_nopiv.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

namespace dopt {
size_t dinv_stride(int nmax) { return (size_t)((nmax + 31) / 32) * 2 * 32 * 32; }
double* dense_dinv(Handle&) { return nullptr; }   // (qp_nopiv_materialize_u: unused here)
// the NLP route's host helpers (unused here)
NLPDims nlp_dims(const Handle&) { return NLPDims{}; }
NLPIn nlp_inputs(const Handle&) { return NLPIn{}; }
NLPRed nlp_red_of(Handle&) { return NLPRed{}; }
}  // namespace dopt
using namespace dopt;

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 1024;
  const int Np = argc > 2 ? atoi(argv[2]) : 320;
  const int ldl = 1;
  const int nmax = Np, ld = Np, n = Np;
  std::vector<double> hQ((size_t)B * n * n);
  unsigned s = 12345;
  for (int b = 0; b < B; ++b) {
    double* Q = hQ.data() + (size_t)b * n * n;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) {
        s = s * 1103515245u + 12345u;
        const double v = ((s >> 8) & 0xffff) / 65536.0 - 0.5;
        Q[(size_t)i * n + j] = Q[(size_t)j * n + i] = v;
      }
    for (int i = 0; i < n; ++i) Q[(size_t)i * n + i] += n;
  }
  std::vector<QPMeta> hm(B);
  for (auto& mm : hm) { mm = {}; mm.nsys = Np; mm.nk = 0; mm.iterative = 0; mm.lu = LU_NONE; mm.sym = 1; }
  double *Q, *K, *dinv, *binv, *ukp, *kamax, *qmax;
  int32_t *perm, *qflag;
  QPMeta* meta;
  hipMalloc(&Q, hQ.size() * 8);
  hipMalloc(&K, (size_t)B * nmax * ld * 8);
  hipMalloc(&dinv, (size_t)B * dinv_stride(nmax) * 8);
  hipMalloc(&binv, (size_t)2 * B * BSTR * 8);
  hipMalloc(&ukp, (size_t)B * nmax * 8);
  hipMalloc(&perm, (size_t)B * nmax * 4);
  hipMalloc(&meta, B * sizeof(QPMeta));
  hipMalloc(&kamax, B * 8);
  hipMalloc(&qmax, B * 8);
  hipMalloc(&qflag, B * 4);
  hipMemcpy(Q, hQ.data(), hQ.size() * 8, hipMemcpyHostToDevice);
  hipMemset(kamax, 0, B * 8);
  hipMemset(qmax, 0, B * 8);
  hipMemset(qflag, 0, B * 4);
  QSrc src{};
  src.Q = Q;
  src.gk = Q;
  src.kls = nullptr;
  src.A = Q;
  src.qmax = qmax;
  src.qflag = qflag;
  src.n = n;
  src.m = 0;
  src.p = 0;
  src.B = B;
  const int nb = (Np + 63) / 64;
  std::vector<hipEvent_t> ev(2 * nb + 1);
  for (auto& e : ev) hipEventCreate(&e);
  std::vector<double> tsum(2 * nb, 0.0);
  std::vector<unsigned long long> st((size_t)B * 16);
  std::vector<double> stsum((size_t)nb * 16, 0.0);
  const int reps = 10;
#ifdef LDIAG_PLACE
  if (B > 4096) return 1;   // ld_place holds 4096 workgroups
  const unsigned mode = argc > 3 ? (unsigned)atoi(argv[3]) : 0u;
  std::vector<unsigned> pl((size_t)B * 16);
  // field layout (gfx9 family; check against the raw values printed below):
  // HW_ID simd [5:4], cu / sh / se [15:8]; LDS_ALLOC base [7:0] (read as [11:0])
  auto cu_of = [&](int b) { return ((unsigned long long)pl[(size_t)b * 16 + 2] << 32) | (pl[(size_t)b * 16] & 0xff00u); };
  auto base_of = [&](int b) { return pl[(size_t)b * 16 + 1] & 0xfffu; };
  auto read_place = [&] {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(pl.data(), HIP_SYMBOL(ld_place), (size_t)B * 16 * 4);
  };
  unsigned cfg[2] = {0u, 1u};
  hipMemcpyToSymbol(HIP_SYMBOL(probe_role_cfg), cfg, sizeof(cfg));
  {
    // one launch with the product's roles: the LDS-base step between the
    // workgroups sharing a CU sizes the slot
    hipMemcpy(meta, hm.data(), B * sizeof(QPMeta), hipMemcpyHostToDevice);
    hipLaunchKernelGGL((nlu_ldiag_kernel<QSrc>), dim3(B), dim3(PNT), 0, 0, K, ld, nmax, perm, dinv, dinv_stride(nmax),
                       meta, 0, binv, ukp, nullptr, nullptr, kamax, nullptr, n, 0, src, 0);
    read_place();
    std::map<unsigned long long, std::set<unsigned>> bases;
    for (int b = 0; b < B; ++b) bases[cu_of(b)].insert(base_of(b));
    unsigned step = 0;
    for (auto& kv : bases) {
      unsigned prev = 0;
      bool first = true;
      for (unsigned v : kv.second) {
        if (!first && (step == 0 || v - prev < step)) step = v - prev;
        prev = v;
        first = false;
      }
    }
    printf("placement: %zu CUs hold the %d workgroups; smallest LDS-base step on a CU %u\n", bases.size(), B, step);
    for (int b = 0; b < B && b < 4; ++b)
      for (int w = 0; w < 4; ++w)
        printf("  raw wg %d wave %d: HW_ID %08x LDS_ALLOC %08x XCC_ID %08x role %u\n", b, w, pl[(size_t)b * 16 + 4 * w],
               pl[(size_t)b * 16 + 4 * w + 1], pl[(size_t)b * 16 + 4 * w + 2], pl[(size_t)b * 16 + 4 * w + 3]);
    if (mode && step == 0) {
      printf("no two workgroups share a CU: the slot is 0, roles = SIMD id\n");
      step = 0xfff + 1;
    }
    cfg[0] = mode;
    cfg[1] = step ? step : 1u;
    hipMemcpyToSymbol(HIP_SYMBOL(probe_role_cfg), cfg, sizeof(cfg));
  }
#endif
  for (int r = 0; r <= reps; ++r) {
    hipMemcpy(meta, hm.data(), B * sizeof(QPMeta), hipMemcpyHostToDevice);
    hipDeviceSynchronize();
    int e = 0;
    hipEventRecord(ev[e++]);
    for (int c0 = 0, J = 0; c0 < Np; c0 += 64, ++J) {
      double* bv = binv + (size_t)(J & 1) * B * BSTR;
      hipLaunchKernelGGL((nlu_ldiag_kernel<QSrc>), dim3(B), dim3(PNT), 0, 0, K, ld, nmax, perm, dinv,
                         dinv_stride(nmax), meta, c0, bv, ukp, nullptr, nullptr, kamax, nullptr, n, 0, src, 0);
      hipEventRecord(ev[e++]);
#ifdef LDIAG_PLACE
      if (r == reps && J == 0) {
        read_place();
        // per CU and phase q: the SIMDs of the role == q waves of its workgroups
        std::map<unsigned long long, std::vector<int>> wgs;
        for (int b = 0; b < B; ++b) wgs[cu_of(b)].push_back(b);
        int shared_simd = 0, dup_role = 0, hist[4][5] = {}, per_cu[8] = {};
        for (int b = 0; b < B; ++b) {
          std::set<unsigned> sd, rl;
          for (int w = 0; w < 4; ++w) {
            sd.insert((pl[(size_t)b * 16 + 4 * w] >> 4) & 3);
            rl.insert(pl[(size_t)b * 16 + 4 * w + 3]);
          }
          shared_simd += sd.size() != 4;
          dup_role += rl.size() != 4;
        }
        for (auto& kv : wgs) {
          per_cu[std::min<size_t>(kv.second.size(), 7)]++;
          for (unsigned q = 0; q < 4; ++q) {
            std::set<unsigned> sd;
            for (int b : kv.second)
              for (int w = 0; w < 4; ++w)
                if (pl[(size_t)b * 16 + 4 * w + 3] == q) sd.insert((pl[(size_t)b * 16 + 4 * w] >> 4) & 3);
            hist[q][std::min<size_t>(sd.size(), 4)]++;
          }
        }
        printf("role mode %u: workgroups whose waves share a SIMD %d, with a repeated role %d\n", mode, shared_simd, dup_role);
        printf("CUs by resident workgroups:");
        for (int k = 1; k < 8; ++k) printf(" %d:%d", k, per_cu[k]);
        printf("\n");
        for (int q = 0; q < 4; ++q)
          printf("phase %d: CUs whose role == %d waves sit on 1 / 2 / 3 / 4 distinct SIMDs: %d / %d / %d / %d\n", q, q,
                 hist[q][1], hist[q][2], hist[q][3], hist[q][4]);
      }
#endif
#ifdef LDIAG_STAMPS
      if (r == reps) {
        hipDeviceSynchronize();
        hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(ld_stamps), (size_t)B * 16 * 8);
        for (int b = 0; b < B; ++b)
          for (int k = 1; k < 11; ++k) {
            const unsigned long long t0 = st[(size_t)b * 16], tk = st[(size_t)b * 16 + k];
            if (tk > t0) stsum[(size_t)J * 16 + k] += (double)(tk - t0) / B;
          }
      }
#endif
      const int ntile = (Np - c0 - 64 + 63) / 64;
      if (ntile > 0) {
        const int tot = ntile * B;
        hipLaunchKernelGGL((nlu_lcol_kernel<QSrc>), dim3(tot), dim3(256), 0, 0, K, ld, nmax, meta, c0, bv, ukp,
                           ntile, tot, kamax, nullptr, n, 0, src);
      }
      hipEventRecord(ev[e++]);
    }
    hipDeviceSynchronize();
    if (r)
      for (int k = 0; k + 1 < e; ++k) {
        float ms;
        hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
        tsum[k] += ms;
      }
  }
  for (int J = 0; J < nb; ++J) {
    printf("B=%d Np=%d ldl=%d J=%d  ldiag %8.2f us  lcol %8.2f us\n", B, Np, ldl, J, 1e3 * tsum[2 * J] / reps,
           1e3 * tsum[2 * J + 1] / reps);
#ifdef LDIAG_STAMPS
    printf("   stamps (cycles from entry):");
    for (int k = 1; k < 11; ++k) printf(" %d:%.0f", k, stsum[(size_t)J * 16 + k]);
    printf("\n");
#endif
  }
  hipMemcpy(hm.data(), meta, B * sizeof(QPMeta), hipMemcpyDeviceToHost);
  int rej = 0;
  for (auto& mm : hm) rej += mm.lu == LU_REJECT;
  printf("  rejected %d\n", rej);
  return 0;
}
