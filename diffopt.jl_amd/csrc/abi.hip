// C-ABI entry points (include/diffopt_mi355x.h).  Every function catches the
// engine's exceptions and maps them onto the header's return-code contract.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "dopt_internal.h"

using dopt::DevBuf;
using dopt::Error;
using dopt::Handle;

struct dopt_handle : public Handle {};

namespace {

template <class F>
int guarded(dopt_handle* h, F&& f) {
  if (!h) return -1;
  try {
    h->err.clear();
    DOPT_CHECK_HIP(hipSetDevice(h->device));
    return f();
  } catch (const Error& e) {
    h->err = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    h->err = e.what();
    return -3;
  }
}

// Host mode: copy `count` doubles of `src` into `buf`; device mode: borrow.
const double* stage_in(Handle& h, DevBuf& buf, const double* src, size_t count) {
  if (!src) return nullptr;
  if (h.mem == DOPT_MEM_DEVICE) return src;
  buf.ensure(count * sizeof(double));
  if (count)
    DOPT_CHECK_HIP(hipMemcpyAsync(buf.p, src, count * sizeof(double), hipMemcpyHostToDevice, h.stream));
  return buf.as<double>();
}

double* out_ptr(Handle& h, DevBuf& buf, double* dst, size_t count) {
  if (!dst) return nullptr;
  if (h.mem == DOPT_MEM_DEVICE) return dst;
  buf.ensure(count * sizeof(double));
  return buf.as<double>();
}

void copy_out(Handle& h, double* dst, const double* dev, size_t count) {
  if (!dst || h.mem == DOPT_MEM_DEVICE || !count) return;
  DOPT_CHECK_HIP(hipMemcpyAsync(dst, dev, count * sizeof(double), hipMemcpyDeviceToHost, h.stream));
}

void wait(Handle& h) { DOPT_CHECK_HIP(hipStreamSynchronize(h.stream)); }

// `bytes` of device memory copied into `dst` (host), waited for
void read_back(Handle& h, void* dst, const void* src, size_t bytes) {
  DOPT_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h.stream));
  wait(h);
}

// A singular problem's info in the coordinates of the reference's LHS
// (QuadraticProgram.jl:256-282, unknowns [z; λ; ν]): the factorised system
// is the reduced one (kept inequality rows only), so a reduced column k maps
// back to z_k, λ_{kidx[k−n]} or ν_{k−n−nk} (1-based).
int full_column(Handle& h, int64_t b, const dopt::QPMeta& mm) {
  const int k = mm.info, n = h.n;
  if (k <= n) return k;
  if (k <= n + mm.nk) {
    int32_t row = 0;
    read_back(h, &row, h.kidx.as<int32_t>() + (size_t)b * h.m + (k - n - 1), sizeof(int32_t));
    return n + row + 1;
  }
  return n + h.m + (k - n - mm.nk);
}

// the factorisation's per-problem metadata, read back
std::vector<dopt::QPMeta> read_meta(Handle& h) {
  std::vector<dopt::QPMeta> meta(h.batch);
  read_back(h, meta.data(), h.meta.p, h.batch * sizeof(dopt::QPMeta));
  return meta;
}

int first_info(Handle& h) {
  const std::vector<dopt::QPMeta> meta = read_meta(h);
  for (int64_t b = 0; b < h.batch; ++b)
    if (!meta[b].iterative && meta[b].info > 0) return full_column(h, b, meta[b]);
  return 0;
}

struct Timer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double s() const {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
};

// An on-pattern gradient's values through the staging buffers: host mode
// copies the caller's array in first, so that the entries no problem's range
// covers come back as they were
double* nz_out_ptr(Handle& h, DevBuf& buf, double* dst, size_t count) {
  if (!dst || h.mem == DOPT_MEM_DEVICE) return dst;
  buf.ensure(std::max<size_t>(count, 1) * sizeof(double));
  if (count) DOPT_CHECK_HIP(hipMemcpyAsync(buf.p, dst, count * sizeof(double), hipMemcpyHostToDevice, h.stream));
  return buf.as<double>();
}

// One call through the staging buffers.  `in` / `out` list the arrays that
// take part: the caller's pointer (host or device by the handle's memory
// mode; null: absent), its slot in tin[] / tout[], and its doubles per seed;
// k seeds scale every count.  `call` gets the device pointers in list order;
// the copies in are queued before it and the copies out after it.  How the
// call ends (a wait, first_info, csc_err_wait, a stream-ordered return) is the
// entry's own.
struct In {
  const double* p;
  int slot;
  size_t count;
};
struct Out {
  double* p;
  int slot;
  size_t count;
  bool keep = false;   // an on-pattern gradient: the caller's values go in first (nz_out_ptr)
};
template <class T, int N>
struct Args {
  T v[N];
  int n = 0;
  Args() = default;
  Args(std::initializer_list<T> l) {
    for (const T& a : l) v[n++] = a;
  }
};
using Ins = Args<In, 7>;
using Outs = Args<Out, 6>;
template <class F>
void staged_call(Handle& h, size_t k, const Ins& in, const Outs& out, F&& call) {
  const double* ip[7];
  double* op[6];
  for (int i = 0; i < in.n; ++i) ip[i] = stage_in(h, h.tin[in.v[i].slot], in.v[i].p, k * in.v[i].count);
  for (int i = 0; i < out.n; ++i) {
    const Out& a = out.v[i];
    op[i] = (a.keep ? nz_out_ptr : out_ptr)(h, h.tout[a.slot], a.p, k * a.count);
  }
  call(ip, op);
  for (int i = 0; i < out.n; ++i) copy_out(h, out.v[i].p, op[i], k * out.v[i].count);
}

// The seed (slot 0; null: none) and the six tangents (slots 1-6) of a QP call
Ins qp_ins(const Handle& h, const double* dl_dz, const double* dQ, const double* dq, const double* dG,
           const double* dh, const double* dA, const double* db) {
  const size_t B = h.batch, n = h.n, m = h.m, p = h.p;
  return {{dl_dz, 0, B * n}, {dQ, 1, B * n * n}, {dq, 2, B * n}, {dG, 3, B * m * n},
          {dh, 4, B * m},    {dA, 5, B * p * n}, {db, 6, B * p}};
}
// ... and the tangents as the kernels take them, from six device pointers:
// G's and A's are absent when the model has no such rows
dopt::FwdTangents fwd_tangents(const Handle& h, const double* const* t) {
  return {t[0], t[1], h.m ? t[2] : nullptr, h.m ? t[3] : nullptr, h.p ? t[4] : nullptr, h.p ? t[5] : nullptr};
}

}  // namespace

extern "C" {

int dopt_abi_version(void) { return DOPT_ABI_VERSION; }

int dopt_create(dopt_handle** out, int device, int64_t batch, int32_t n, int32_t m,
                int32_t p, int32_t kind) {
  if (!out) return -1;
  *out = nullptr;
  if (batch < 0 || n < 0 || m < 0 || p < 0 ||
      (kind != DOPT_KIND_QP && kind != DOPT_KIND_CONIC && kind != DOPT_KIND_NLP))
    return -1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -4;
  if (device < 0 || device >= ndev) return -1;
  auto* h = new dopt_handle();
  h->device = device;
  h->batch = batch;
  h->n = n;
  h->m = m;
  h->p = p;
  h->kind = kind;
  int rc = guarded(h, [&]() {
    DOPT_CHECK_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    if (const char* e = getenv("DOPT_CONIC_SPLIT")) {
      if (e[0] == '0' || e[0] == '1') h->conic_split = e[0] - '0';
    }
    if (const char* e = getenv("DOPT_LU")) h->lu_mode = atoi(e) != 0;
    if (const char* e = getenv("DOPT_SYM")) h->sym_mode = atoi(e) != 0;
    if (const char* e = getenv("DOPT_LEFT")) h->left_mode = atoi(e) != 0;
    if (const char* e = getenv("DOPT_QP_SUMMARY")) h->summary_mode = atoi(e) != 0;
    if (const char* e = getenv("DOPT_NLP_REDUCE")) h->nlp_reduce = atoi(e) != 0;
    if (const char* e = getenv("DOPT_SPLIT_FUSE")) h->split_fuse = atoi(e) != 0;
    if (kind == DOPT_KIND_QP) {
      // largest supported system: the generic solve stages an nmax vector in
      // LDS (64 KB); the blocked route takes reduced systems up to BLOCKED_MAX
      // above the dense route's cap (8192: the generic solve stages an nmax
      // vector in LDS) the handle takes the sparse route (sparse.hip): the MOI
      // matrix form through dopt_qp_set_csc, the LSQR branch, no dense K
      if ((int64_t)n + m + p > dopt::DENSE_QP_MAX) {
        h->sparse = true;
        h->kamax.ensure(sizeof(double));
        return 0;
      }
      // Systems are identity-padded to whole 32-column blocks (qp_assemble.hip),
      // so the per-problem stride / row stride are rounded up to 32.
      h->nmax = (int32_t)dopt::round_up(std::max(n + m + p, 1), 32);
      h->ld = h->nmax;
      h->K.ensure((size_t)batch * h->nmax * h->ld * sizeof(double));
      h->ipiv.ensure((size_t)batch * std::max(h->nmax, 1) * sizeof(int32_t));
      h->s.ensure((size_t)batch * std::max(m, 1) * sizeof(double));
      h->kidx.ensure((size_t)2 * batch * std::max(m, 1) * sizeof(int32_t));
      h->kls.ensure((size_t)2 * batch * std::max(m, 1) * sizeof(double));
      h->gk.ensure((size_t)batch * std::max(n, 1) * std::max(m, 1) * sizeof(double));
      h->meta.ensure((size_t)std::max<int64_t>(batch, 1) * sizeof(dopt::QPMeta));
      h->kamax.ensure((size_t)std::max<int64_t>(batch, 1) * sizeof(double));
      // rhs: [reverse RHS | full forward RHS | reduced forward RHS]; x: [reverse | forward]
      h->rhs.ensure((size_t)3 * batch * std::max(h->nmax, 1) * sizeof(double));
      h->x.ensure((size_t)2 * batch * std::max(h->nmax, 1) * sizeof(double));
    }
    return 0;
  });
  if (rc != 0) {
    dopt_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int dopt_destroy(dopt_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->aux) {
    (void)hipStreamSynchronize(h->aux);
    (void)hipStreamDestroy(h->aux);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_qsym) (void)hipEventDestroy(h->ev_qsym);
  if (h->ev_crit) (void)hipEventDestroy(h->ev_crit);
  if (h->crit) {
    (void)hipStreamSynchronize(h->crit);
    (void)hipStreamDestroy(h->crit);
  }
  for (auto& pe : h->ev_pending) {
    (void)hipEventDestroy(pe.second.first);
    (void)hipEventDestroy(pe.second.second);
  }
  for (auto e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->meta_host) (void)hipHostFree(h->meta_host);
  if (h->qsum) (void)hipHostFree(h->qsum);
  if (h->pin_ev) (void)hipEventDestroy(h->pin_ev);
  if (h->meta_ev) (void)hipEventDestroy(h->meta_ev);
  if (h->meta_fork) (void)hipEventDestroy(h->meta_fork);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // every DevBuf and PinBuf frees itself
  return 0;
}

int64_t dopt_live_device_bytes(void) { return dopt::live_device_bytes.load(); }

const char* dopt_last_error(const dopt_handle* h) { return h ? h->err.c_str() : "null handle"; }

int dopt_set_stream(dopt_handle* h, void* stream) {
  return guarded(h, [&]() {
    wait(*h);
    if (h->own_stream && h->stream) DOPT_CHECK_HIP(hipStreamDestroy(h->stream));
    h->own_stream = false;
    h->stream = static_cast<hipStream_t>(stream);  // NULL = legacy default stream
    return 0;
  });
}

int dopt_set_memory(dopt_handle* h, int32_t mem) {
  return guarded(h, [&]() {
    if (mem != DOPT_MEM_HOST && mem != DOPT_MEM_DEVICE) throw Error(-1, "bad memory mode");
    h->mem = mem;
    return 0;
  });
}

int dopt_set_sparse(dopt_handle* h, int32_t on) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP && h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_set_sparse: QP and conic handles only");
    if (h->kind == DOPT_KIND_CONIC) {   // A_moi kept sparse by dopt_conic_set_csc: the persistent LSQR on it,
      h->sparse = on != 0;              // or (DOPT_SPARSE_SPLIT) the split LSQR
      h->sparse_split = on == DOPT_SPARSE_SPLIT;
      h->cset = h->cfactored = false;
      return 0;
    }
    if (!on && (int64_t)h->n + h->m + h->p > dopt::DENSE_QP_MAX)
      throw Error(-1, "dopt_set_sparse: n + m + p > 8192 has only the sparse route");
    h->sparse = on != 0;
    h->set = h->factored = h->small_ready = false;   // a model is set again under the new route
    return 0;
  });
}

int dopt_qp_set(dopt_handle* h, const double* Q, const double* G, const double* hv,
                const double* A, const double* z, const double* lam, const double* nu) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_set on a non-QP handle");
    if (h->sparse) throw Error(-1, "dopt_qp_set: a sparse-route handle takes the MOI matrix form (dopt_qp_set_csc)");
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p;
    if (!Q || !z) throw Error(-1, "Q and z are required");
    if (m && (!G || !hv || !lam)) throw Error(-1, "G, h and lam are required when m > 0");
    if (p && (!A || !nu)) throw Error(-1, "A and nu are required when p > 0");
    // the staging below may reallocate the buffers the previous model's
    // pointers name: the handle holds no model until this call succeeds
    h->set = false;
    h->factored = false;
    h->small_ready = false;
    h->Q = stage_in(*h, h->own_in[0], Q, B * n * n);
    h->G = m ? stage_in(*h, h->own_in[1], G, B * m * n) : nullptr;
    h->hv = m ? stage_in(*h, h->own_in[2], hv, B * m) : nullptr;
    h->A = p ? stage_in(*h, h->own_in[3], A, B * p * n) : nullptr;
    h->z = stage_in(*h, h->own_in[4], z, B * n);
    h->lam = m ? stage_in(*h, h->own_in[5], lam, B * m) : nullptr;
    h->nu = p ? stage_in(*h, h->own_in[6], nu, B * p) : nullptr;
    h->set = true;
    h->factored = false;
    wait(*h);
    return 0;
  });
}

// Host mode: copy `count` int64 of `src` into `buf`; device mode: borrow.
static const int64_t* stage_in_i64(Handle& h, DevBuf& buf, const int64_t* src, size_t count) {
  if (!src) return nullptr;
  if (h.mem == DOPT_MEM_DEVICE) return src;
  buf.ensure(std::max<size_t>(count, 1) * sizeof(int64_t));
  if (count)
    DOPT_CHECK_HIP(hipMemcpyAsync(buf.p, src, count * sizeof(int64_t), hipMemcpyHostToDevice, h.stream));
  return (const int64_t*)buf.p;
}

// Host-mode inputs of at most PACK_MAX bytes in all: gathered into the
// handle's pinned buffer (memcpy) and moved by one host→device copy, the
// device pointers returned in order (null stays null).  Larger inputs keep
// one copy per array (a host memcpy of gigabytes costs more than it saves).
constexpr size_t PACK_MAX = (size_t)8 << 20;
constexpr size_t LHS_PACK_MAX = (size_t)1 << 20;   // dopt_lhs_solve: M and the sides (the host memcpy pays below)
struct PackIn {
  const void* src;
  size_t bytes;
};
static bool pack_in(Handle& h, const PackIn* in, int k, const void** out, DevBuf* dst = nullptr) {
  if (h.mem == DOPT_MEM_DEVICE) return false;
  if (h.pin_pending) {   // a set_csc's copy out of the buffer may still be queued
    DOPT_CHECK_HIP(hipEventSynchronize(h.pin_ev));
    h.pin_pending = false;
  }
  DevBuf& D = dst ? *dst : h.pack;
  size_t tot = 0;
  for (int i = 0; i < k; ++i) tot += (in[i].bytes + 15) & ~(size_t)15;
  if (tot == 0 || tot > PACK_MAX) return false;
  // the previous call's copy out of the pinned buffer is complete: every
  // host-mode entry point synchronises before it returns
  char* pin = h.pin.grow(tot);
  D.ensure(tot);
  size_t off = 0;
  for (int i = 0; i < k; ++i) {
    if (!in[i].src) {
      out[i] = nullptr;
      continue;
    }
    std::memcpy(pin + off, in[i].src, in[i].bytes);
    out[i] = static_cast<const char*>(D.p) + off;
    off += (in[i].bytes + 15) & ~(size_t)15;
  }
  DOPT_CHECK_HIP(hipMemcpyAsync(D.p, pin, off, hipMemcpyHostToDevice, h.stream));
  return true;
}

// The checks csc_scatter_kernel makes, on the host (a small host-mode model:
// cheaper than reading the device's verdict back): bit 1 a column range out of
// order / bounds, bit 2 a row index out of range.
static int host_csc_check(const int64_t* cp, const int64_t* rv, int64_t nnz, size_t rows, size_t ncols, size_t B) {
  int err = 0;
  for (size_t b = 0; b < B; ++b) {
    const int64_t* c = cp + b * (ncols + 1);
    for (size_t j = 0; j < ncols; ++j) {
      const int64_t k0 = c[j] - 1, k1 = c[j + 1] - 1;
      if (k0 < 0 || k1 < k0 || k1 > nnz) {
        err |= 1;
        continue;
      }
      for (int64_t k = k0; k < k1; ++k) {
        const int64_t r = rv[k] - 1;
        if (r < 0 || r >= (int64_t)rows) err |= 2;
      }
    }
  }
  return err;
}

// Pinned or pageable, asked once per small-path or plug-point call: pinned
// staging pays from a handle's third such call on, or as soon as the pinned
// read-back buffer exists (its hipHostMalloc costs more than the pageable
// copies of a call or two save: a handle per model — LHS then LHS' — stays
// pageable).  Device mode stages nothing.
static bool use_pinned(Handle& h) { return h.mem != DOPT_MEM_DEVICE && (h.pin_out.p || ++h.io_calls >= 3); }

// The transport of one small-path call (qp_small.hip): `nin` inputs (the seed
// or the tangents; null: absent), `ob` bytes of outputs and `fb` bytes of
// per-problem flags (0: the call has none).  The constructor yields the device
// pointers to launch with, finish() waits and yields the host's view.
//   pinned, in place   host mode, use_pinned, no matrix input: the kernel reads
//                      the inputs from and writes [outputs | flags] to pin_out
//   pinned, packed     ... a matrix input: the inputs by one copy (pack_in into
//                      tpack), [outputs | flags] written to pin_out
//   pageable           host mode otherwise (a handle's first calls, or inputs
//                      the pack refuses): tin[slot + i] / tout[slot], one copy
//                      each way
//   borrowed           device mode: the caller's arrays; the flags in csc_err
// (the previous call's use of pin_out is complete: every entry point that
// uses it waits before it returns)
struct SmallIO {
  Handle& h;
  const size_t ob, fb;
  const bool host;
  bool pinned;
  const double* in[6] = {};
  double* out = nullptr;
  int32_t* flags = nullptr;
  std::vector<char> page;
  const char* view = nullptr;   // after finish(): [outputs | flags] on the host (device mode: the flags alone)

  SmallIO(Handle& hh, const PackIn* src, int nin, bool matrix_in, int slot, double* dst, size_t obytes, size_t fbytes)
      : h(hh), ob(obytes), fb(fbytes), host(hh.mem != DOPT_MEM_DEVICE), pinned(use_pinned(hh)) {
    const void* pd[6];
    if (pinned && matrix_in) pinned = pack_in(h, src, nin, pd, &h.tpack);
    char* dev = nullptr;
    if (pinned && matrix_in) {
      for (int i = 0; i < nin; ++i) in[i] = static_cast<const double*>(pd[i]);
      h.pin_out.grow(ob + fb);
      dev = h.pin_out.dev;
    } else if (pinned) {
      size_t off[6], tot = (ob + fb + 15) & ~(size_t)15;
      for (int i = 0; i < nin; ++i) off[i] = tot, tot += (src[i].bytes + 15) & ~(size_t)15;
      char* pz = h.pin_out.grow(tot);
      dev = h.pin_out.dev;
      for (int i = 0; i < nin; ++i) {
        if (!src[i].src) continue;
        std::memcpy(pz + off[i], src[i].src, src[i].bytes);
        in[i] = reinterpret_cast<const double*>(dev + off[i]);
      }
    } else if (host) {
      for (int i = 0; i < nin; ++i)
        in[i] = stage_in(h, h.tin[slot + i], static_cast<const double*>(src[i].src), src[i].bytes / sizeof(double));
      h.tout[slot].ensure(ob + fb);
      dev = h.tout[slot].as<char>();
    } else {
      for (int i = 0; i < nin; ++i) in[i] = static_cast<const double*>(src[i].src);
      out = dst;
      h.csc_err.ensure(fb);
      flags = fb ? h.csc_err.as<int32_t>() : nullptr;
      return;
    }
    out = reinterpret_cast<double*>(dev);
    flags = fb ? reinterpret_cast<int32_t*>(dev + ob) : nullptr;
  }
  // waits for the launch; true: no problem raised a flag
  bool finish() {
    if (pinned) {
      view = h.pin_out.p;
      wait(h);
    } else {
      page.resize(host ? ob + fb : fb);
      if (!page.empty())
        DOPT_CHECK_HIP(hipMemcpyAsync(page.data(), host ? static_cast<const void*>(out) : flags, page.size(),
                                      hipMemcpyDeviceToHost, h.stream));
      wait(h);
      view = page.data();
    }
    const int32_t* hf = reinterpret_cast<const int32_t*>(view + (host ? ob : 0));
    return std::all_of(hf, hf + fb / sizeof(int32_t), [](int32_t f) { return f == 0; });
  }
  void deliver(double* dst) const {
    if (host) std::memcpy(dst, view, ob);
  }
};

// The solution of a packed plug-point call (dopt_lhs_solve / _resolve): one
// copy into the pinned read-back buffer, then the caller's array
static void pinned_copy_out(Handle& h, double* dst, const double* dev, size_t count) {
  char* pin = h.pin_out.grow(count * sizeof(double));
  read_back(h, pin, dev, count * sizeof(double));
  std::memcpy(dst, pin, count * sizeof(double));
}

// the message of a CSC setter's error word (bit 1: colptr, bit 2: rowval)
static const char* csc_err_text(int err) {
  return (err & 1) ? "CSC colptr is not monotone / out of range" : "CSC rowval out of range";
}
// ... the device's word (csc_err), read back
static int csc_err_read(Handle& h) {
  int herr = 0;
  read_back(h, &herr, h.csc_err.p, sizeof(int));
  return herr;
}

int dopt_qp_set_csc(dopt_handle* h,
                    const int64_t* Q_colptr, const int64_t* Q_rowval, const double* Q_nzval, int64_t Q_nnz,
                    const int64_t* G_colptr, const int64_t* G_rowval, const double* G_nzval, int64_t G_nnz,
                    const int64_t* A_colptr, const int64_t* A_rowval, const double* A_nzval, int64_t A_nnz,
                    const double* hv, const double* z, const double* lam, const double* nu) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_set_csc on a non-QP handle");
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p;
    if (!Q_colptr || !z) throw Error(-1, "Q and z are required");
    if (m && (!G_colptr || !hv || !lam)) throw Error(-1, "G, h and lam are required when m > 0");
    if (p && (!A_colptr || !nu)) throw Error(-1, "A and nu are required when p > 0");
    if (Q_nnz < 0 || G_nnz < 0 || A_nnz < 0) throw Error(-1, "nnz must be >= 0");
    if ((Q_nnz > 0 && (!Q_rowval || !Q_nzval)) || (m && G_nnz > 0 && (!G_rowval || !G_nzval)) ||
        (p && A_nnz > 0 && (!A_rowval || !A_nzval)))
      throw Error(-1, "rowval and nzval are required when nnz > 0");
    // every host-side check is done: from here on the staging may reallocate
    // (or overwrite) the buffers the previous model's pointers name, so the
    // handle holds no model until this call succeeds
    h->set = false;
    h->factored = false;
    h->small_ready = false;
    // a throw after a queued copy out of the pinned buffer waits for it, so
    // the next call's memcpy into that buffer cannot race the DMA
    struct SyncOnThrow {
      hipStream_t s;
      ~SyncOnThrow() {
        if (std::uncaught_exceptions() > 0) (void)hipStreamSynchronize(s);
      }
    } sync_on_throw{h->stream};
    h->csc_err.ensure(sizeof(int));
    int* err = h->csc_err.as<int>();
    // Q, G, A: absent (no rows) matrices have no arrays, empty ones only a colptr
    struct Mat { const int64_t *cp, *rv; const double* nz; int64_t nnz; size_t rows; int slot; };
    Mat mats[3] = {{Q_colptr, Q_rowval, Q_nzval, Q_nnz, n, 0},
                   {G_colptr, G_rowval, G_nzval, G_nnz, m, 1},
                   {A_colptr, A_rowval, A_nzval, A_nnz, p, 3}};
    for (Mat& M : mats) {
      if (!M.rows) M.cp = nullptr;
      if (!M.rows || !M.nnz) M.rv = nullptr, M.nz = nullptr;
    }
    // one matrix's arrays, each by its own copy (device mode: borrowed)
    auto stage_mat = [&](int k) {
      const Mat& M = mats[k];
      return dopt::CscArg{stage_in_i64(*h, h->csc_in[3 * k], M.cp, B * (n + 1)),
                          stage_in_i64(*h, h->csc_in[3 * k + 1], M.rv, (size_t)M.nnz),
                          stage_in(*h, h->csc_in_val[k], M.nz, (size_t)M.nnz), M.nnz};
    };
    auto stage_vectors = [&]() {
      h->hv = m ? stage_in(*h, h->own_in[2], hv, B * m) : nullptr;
      h->z = stage_in(*h, h->own_in[4], z, B * n);
      h->lam = m ? stage_in(*h, h->own_in[5], lam, B * m) : nullptr;
      h->nu = p ? stage_in(*h, h->own_in[6], nu, B * p) : nullptr;
    };
    if (h->sparse) {   // kept sparse (sparse.hip): G, A and their CSR copies; Q only tested for zero
      DOPT_CHECK_HIP(hipMemsetAsync(h->csc_err.p, 0, sizeof(int), h->stream));
      const dopt::CscArg Q = stage_mat(0), G = stage_mat(1), A = stage_mat(2);
      dopt::sp_set_csc(*h, Q.cp, Q.rv, Q.nz, Q.nnz, G.cp, G.rv, G.nz, G.nnz, A.cp, A.rv, A.nz, A.nnz, err);
      const int herr = csc_err_read(*h);
      if (herr & 3) throw Error(-1, csc_err_text(herr));
      h->sp_qnz = (herr & 4) != 0;
      h->Q = h->G = h->A = nullptr;
      stage_vectors();
      h->set = true;
      wait(*h);
      return 0;
    }
    // small models (the Julia back-end's batch of one): every array in one copy
    PackIn pin[13];
    const void* pdev[13];
    for (int k = 0; k < 3; ++k) {
      const Mat& M = mats[k];
      const bool on = M.rows > 0;
      pin[3 * k] = {M.cp, on ? B * (n + 1) * sizeof(int64_t) : 0};
      pin[3 * k + 1] = {M.rv, on ? (size_t)M.nnz * sizeof(int64_t) : 0};
      pin[3 * k + 2] = {M.nz, on ? (size_t)M.nnz * sizeof(double) : 0};
    }
    pin[9] = {m ? hv : nullptr, m ? B * m * sizeof(double) : 0};
    pin[10] = {z, B * n * sizeof(double)};
    pin[11] = {m ? lam : nullptr, m ? B * m * sizeof(double) : 0};
    pin[12] = {p ? nu : nullptr, p ? B * p * sizeof(double) : 0};
    // a packed (small host-mode) model is validated here, so the call returns
    // with its copy and scatter queued instead of reading the device's verdict
    int hostv = -1;
    size_t pbytes = 0;
    for (const PackIn& q : pin) pbytes += q.bytes;
    if (h->mem != DOPT_MEM_DEVICE && pbytes <= PACK_MAX / 2) {
      hostv = 0;
      for (const Mat& M : mats)
        if (M.rows > 0) hostv |= host_csc_check(M.cp, M.rv, M.nnz, M.rows, n, B);
      if (hostv) throw Error(-1, csc_err_text(hostv));
    }
    const bool packed = pack_in(*h, pin, 13, pdev);
    const bool async = packed && hostv == 0;
    if (!async) DOPT_CHECK_HIP(hipMemsetAsync(h->csc_err.p, 0, sizeof(int), h->stream));
    const double* dense[3] = {nullptr, nullptr, nullptr};
    dopt::CscTriple T{};
    for (int k = 0; k < 3; ++k) {
      const Mat& M = mats[k];
      if (M.rows == 0) continue;
      const dopt::CscArg a = packed ? dopt::CscArg{(const int64_t*)pdev[3 * k], (const int64_t*)pdev[3 * k + 1],
                                                   (const double*)pdev[3 * k + 2], M.nnz}
                                    : stage_mat(k);
      DevBuf& d = h->own_in[M.slot];
      d.ensure(B * M.rows * n * sizeof(double));
      dense[k] = d.as<double>();
      if (async) {   // validated on the host: Q, G and A zero-filled and scattered by ONE launch (below)
        T.cp[k] = a.cp, T.rv[k] = a.rv, T.nz[k] = a.nz, T.dense[k] = d.as<double>(), T.rows[k] = (int)M.rows;
      } else {
        dopt::csc_to_dense(*h, a.cp, a.rv ? a.rv : a.cp, a.nz ? a.nz : (const double*)d.p, M.nnz, (int)M.rows,
                           (int)n, d.as<double>(), err);
      }
    }
    if (async) {
      dopt::csc_to_dense3(*h, T);
    } else if (const int herr = csc_err_read(*h)) {
      throw Error(-1, csc_err_text(herr));
    }
    h->Q = dense[0];
    h->G = m ? dense[1] : nullptr;
    h->A = p ? dense[2] : nullptr;
    if (packed) {   // the pack stays as the inputs' home until the next set
      h->hv = (const double*)pdev[9];
      h->z = (const double*)pdev[10];
      h->lam = (const double*)pdev[11];
      h->nu = (const double*)pdev[12];
    } else {
      stage_vectors();
    }
    h->set = true;
    h->factored = false;
    if (async) {   // the inputs are in the pinned buffer: nothing of the caller's is read later
      if (!h->pin_ev) DOPT_CHECK_HIP(hipEventCreateWithFlags(&h->pin_ev, hipEventDisableTiming));
      DOPT_CHECK_HIP(hipEventRecord(h->pin_ev, h->stream));
      h->pin_pending = true;
      return 0;
    }
    wait(*h);
    return 0;
  });
}

int dopt_qp_factor(dopt_handle* h) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_factor on a non-QP handle");
    if (h->sparse) {
      dopt::sp_factor(*h);
      return 0;
    }
    dopt::qp_factor(*h);
    return first_info(*h);
  });
}

int dopt_qp_reverse_grads(dopt_handle* h, const double* rev, double* dQ, double* dq, double* dG,
                          double* g_const, double* dA, double* a_const) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_reverse_grads on a non-QP handle");
    if (!rev) throw Error(-1, "rev is required");
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p;
    staged_call(*h, 1, {{rev, 0, B * L}},
                {{dQ, 0, B * n * n}, {dq, 1, B * n}, {dG, 2, B * m * n}, {g_const, 3, B * m}, {dA, 4, B * p * n},
                 {a_const, 5, B * p}},
                [&](const double** i, double** o) { dopt::qp_reverse_grads(*h, i[0], o[0], o[1], o[2], o[3], o[4], o[5]); });
    wait(*h);
    return 0;
  });
}

int dopt_qp_params_reverse(dopt_handle* h, const double* rev, int32_t nparam, int64_t nterms,
                           const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                           const double* t_coef, double* out_dp) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_params_reverse on a non-QP handle");
    if (!rev || (nparam > 0 && !out_dp)) throw Error(-1, "rev and out_dp are required");
    const size_t B = h->batch, L = (size_t)h->n + h->m + h->p, P = nparam > 0 ? (size_t)nparam : 0;
    staged_call(*h, 1, {{rev, 0, B * L}}, {{P ? out_dp : nullptr, 0, B * P}}, [&](const double** i, double** o) {
      dopt::qp_params_reverse(*h, i[0], nparam, nterms, t_param, t_kind, t_index, t_coef, o[0]);
    });
    wait(*h);
    return 0;
  });
}

int dopt_qp_params_forward(dopt_handle* h, const double* dp, int32_t nparam, int64_t nterms,
                           const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                           const double* t_coef, double* dq, double* dh, double* db) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_params_forward on a non-QP handle");
    if ((nparam > 0 && !dp) || !dq || (h->m && !dh) || (h->p && !db))
      throw Error(-1, "dp, dq, dh (m > 0) and db (p > 0) are required");
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, P = nparam > 0 ? (size_t)nparam : 0;
    staged_call(*h, 1, {{P ? dp : nullptr, 0, B * P}},
                {{dq, 0, B * n}, {m ? dh : nullptr, 1, B * m}, {p ? db : nullptr, 2, B * p}},
                [&](const double** i, double** o) {
                  dopt::qp_params_forward(*h, i[0], nparam, nterms, t_param, t_kind, t_index, t_coef, o[0], o[1], o[2]);
                });
    wait(*h);
    return 0;
  });
}

int dopt_qp_reverse(dopt_handle* h, const double* dl_dz, double* out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_reverse on a non-QP handle");
    if (!dl_dz || !out) throw Error(-1, "dl_dz and out are required");
    Timer tm;
    const size_t B = h->batch, n = h->n, L = h->n + h->m + h->p;
    if (h->sparse) {   // sparse route: LSQR on the implicit LHS (no singular verdict)
      staged_call(*h, 1, {{dl_dz, 0, B * n}}, {{out, 0, B * L}},
                  [&](const double** i, double** o) { dopt::sp_reverse(*h, i[0], o[0]); });
      wait(*h);
      h->last_time = tm.s();
      return 0;
    }
    // a model not yet factorised, batch of a few: the one-launch small path
    // (qp_small.hip) through SmallIO's transport — in host mode from a handle's
    // third call on no copy at all; anything it cannot take (a problem's flag
    // set) runs the batched route below
    const double* staged = nullptr;
    if (!h->factored && dopt::qp_small_eligible(*h)) {
      const PackIn seed[1] = {{dl_dz, B * n * sizeof(double)}};
      SmallIO io(*h, seed, 1, false, 0, out, B * L * sizeof(double), B * sizeof(int32_t));
      dopt::qp_small_reverse(*h, io.in[0], io.out, io.flags);
      h->small_ready = io.finish();
      if (h->small_ready) {
        io.deliver(out);
        h->last_time = tm.s();
        return 0;
      }
      if (!io.pinned) staged = io.in[0];   // the seed is in tin[0] already (device mode: the caller's)
    }
    double* o = out_ptr(*h, h->tout[0], out, B * L);
    dopt::qp_reverse(*h, staged ? staged : stage_in(*h, h->tin[0], dl_dz, B * n), o);
    copy_out(*h, out, o, B * L);
    const int rc = first_info(*h);
    h->last_time = tm.s();
    return rc;
  });
}

int dopt_qp_forward(dopt_handle* h, const double* dQ, const double* dq, const double* dG,
                    const double* dh, const double* dA, const double* db, double* out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_forward on a non-QP handle");
    if (!out) throw Error(-1, "out is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p;
    // the small path's factors (dopt_qp_reverse).  Vector tangents only (dq,
    // dh, db; the matrix ones zero): SmallIO's in-place form, no copy at all;
    // a matrix tangent: one packed copy in
    if (!h->sparse && !h->factored && h->small_ready) {
      const PackIn tan[6] = {{dQ, B * n * n * sizeof(double)}, {dq, B * n * sizeof(double)},
                             {m ? dG : nullptr, B * m * n * sizeof(double)}, {m ? dh : nullptr, B * m * sizeof(double)},
                             {p ? dA : nullptr, B * p * n * sizeof(double)}, {p ? db : nullptr, B * p * sizeof(double)}};
      SmallIO io(*h, tan, 6, tan[0].src || tan[2].src || tan[4].src, 1, out, B * L * sizeof(double), 0);
      dopt::qp_small_forward(*h, fwd_tangents(*h, io.in), io.out);
      io.finish();
      io.deliver(out);
      h->last_time = tm.s();
      return 0;
    }
    int rc = 0;
    staged_call(*h, 1, qp_ins(*h, nullptr, dQ, dq, dG, dh, dA, db), {{out, 1, B * L}},
                [&](const double** i, double** o) {
                  if (h->sparse) dopt::sp_forward(*h, fwd_tangents(*h, i + 1), o[0]);
                  else dopt::qp_forward(*h, i[1], i[2], i[3], i[4], i[5], i[6], o[0]);
                });
    if (h->sparse) wait(*h);
    else rc = first_info(*h);
    h->last_time = tm.s();
    return rc;
  });
}

int dopt_qp_reverse_k(dopt_handle* h, int32_t k, const double* dl_dz, double* out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_reverse_k on a non-QP handle");
    if (h->sparse) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
    if (!dl_dz || !out) throw Error(-1, "dl_dz and out are required");
    if (k <= 0) throw Error(-1, "k must be positive");
    Timer tm;
    const size_t B = h->batch, n = h->n, L = h->n + h->m + h->p;
    staged_call(*h, k, {{dl_dz, 0, B * n}}, {{out, 0, B * L}},
                [&](const double** i, double** o) { dopt::qp_reverse_k(*h, k, i[0], o[0]); });
    const int rc = first_info(*h);
    h->last_time = tm.s();
    return rc;
  });
}

int dopt_qp_forward_k(dopt_handle* h, int32_t k, const double* dQ, const double* dq, const double* dG,
                      const double* dh, const double* dA, const double* db, double* out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_forward_k on a non-QP handle");
    if (h->sparse) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
    if (!out) throw Error(-1, "out is required");
    if (k <= 0) throw Error(-1, "k must be positive");
    Timer tm;
    const size_t L = (size_t)h->n + h->m + h->p;
    staged_call(*h, k, qp_ins(*h, nullptr, dQ, dq, dG, dh, dA, db), {{out, 1, h->batch * L}},
                [&](const double** i, double** o) {
                  dopt::qp_forward_k(*h, k, i[1], i[2], i[3], i[4], i[5], i[6], o[0]);
                });
    const int rc = first_info(*h);
    h->last_time = tm.s();
    return rc;
  });
}

// The parameter calls on k seeds (params.hip): right-hand sides from the term table, the _k solves
int dopt_qp_params_forward_k(dopt_handle* h, int32_t k, const double* dp, int32_t nparam, int64_t nterms,
                             const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                             const int32_t* t_var, const double* t_coef, double* out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_params_forward_k on a non-QP handle");
    if (h->sparse) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
    if (k < 0) throw Error(-1, "k must not be negative");
    if (!dp && k != nparam) throw Error(-1, "dopt_qp_params_forward_k: unit seeds (dp == NULL) need k == nparam");
    Timer tm;
    const size_t B = h->batch, L = (size_t)h->n + h->m + h->p, P = nparam > 0 ? (size_t)nparam : 0;
    const bool work = P && k && B;
    staged_call(*h, k, {{work ? dp : nullptr, 0, B * P}}, {{work ? out : nullptr, 1, B * L}},
                [&](const double** i, double** o) {
                  dopt::qp_params_forward_k(*h, k, i[0], nparam, nterms, t_param, t_kind, t_index, t_var, t_coef,
                                            o[0]);
                });
    const int rc = work ? first_info(*h) : 0;
    h->last_time = tm.s();
    return rc;
  });
}

int dopt_qp_params_reverse_k(dopt_handle* h, int32_t k, const double* dl_dz, int32_t nparam, int64_t nterms,
                             const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                             const int32_t* t_var, const double* t_coef, double* out_rev, double* out_dp) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_params_reverse_k on a non-QP handle");
    if (h->sparse) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
    if (k < 0) throw Error(-1, "k must not be negative");
    if (!dl_dz && k != h->n) throw Error(-1, "dopt_qp_params_reverse_k: unit seeds (dl_dz == NULL) need k == n");
    Timer tm;
    const size_t B = h->batch, n = h->n, L = n + h->m + h->p, P = nparam > 0 ? (size_t)nparam : 0;
    const bool work = P && k && B;
    staged_call(*h, k, {{work ? dl_dz : nullptr, 0, B * n}},
                {{work ? out_rev : nullptr, 0, B * L}, {work ? out_dp : nullptr, 1, B * P}},
                [&](const double** i, double** o) {
                  dopt::qp_params_reverse_k(*h, k, i[0], nparam, nterms, t_param, t_kind, t_index, t_var, t_coef,
                                            o[0], o[1]);
                });
    const int rc = work ? first_info(*h) : 0;
    h->last_time = tm.s();
    return rc;
  });
}

// Reverse with seeds on the duals (params.hip; the sparse route: sparse.hip, one seed)
int dopt_qp_reverse_duals_k(dopt_handle* h, int32_t k, const double* dl_dz, const double* dl_dlam,
                            const double* dl_dnu, double* out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_reverse_duals_k on a non-QP handle");
    if (k < 1) throw Error(-1, "k must be positive");
    if (h->sparse && k > 1) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
    if (!out) throw Error(-1, "out is required");
    if (!dl_dz && !dl_dlam && !dl_dnu) throw Error(-1, "dopt_qp_reverse_duals_k: at least one seed block is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p;
    int rc = 0;
    staged_call(*h, k, {{dl_dz, 0, B * n}, {m ? dl_dlam : nullptr, 1, B * m}, {p ? dl_dnu : nullptr, 2, B * p}},
                {{out, 0, B * L}}, [&](const double** i, double** o) {
                  if (h->sparse) dopt::sp_reverse_duals(*h, i[0], i[1], i[2], o[0]);
                  else dopt::qp_reverse_duals_k(*h, k, i[0], i[1], i[2], o[0]);
                });
    if (h->sparse) wait(*h);
    else rc = first_info(*h);
    h->last_time = tm.s();
    return rc;
  });
}

int dopt_qp_params_reverse_duals_k(dopt_handle* h, int32_t k, const double* dl_dz, const double* dl_dlam,
                                   const double* dl_dnu, int32_t nparam, int64_t nterms, const int32_t* t_param,
                                   const int32_t* t_kind, const int32_t* t_index, const int32_t* t_var,
                                   const double* t_coef, double* out_rev, double* out_dp) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_params_reverse_duals_k on a non-QP handle");
    if (h->sparse) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
    if (k < 1) throw Error(-1, "k must be positive");
    if (!dl_dz && !dl_dlam && !dl_dnu)
      throw Error(-1, "dopt_qp_params_reverse_duals_k: at least one seed block is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p, P = nparam > 0 ? (size_t)nparam : 0;
    const bool work = P && B;
    staged_call(*h, k,
                {{work ? dl_dz : nullptr, 0, B * n},
                 {work && m ? dl_dlam : nullptr, 1, B * m},
                 {work && p ? dl_dnu : nullptr, 2, B * p}},
                {{work ? out_rev : nullptr, 0, B * L}, {work ? out_dp : nullptr, 1, B * P}},
                [&](const double** i, double** o) {
                  dopt::qp_params_reverse_duals_k(*h, k, i[0], i[1], i[2], nparam, nterms, t_param, t_kind, t_index,
                                                  t_var, t_coef, o[0], o[1]);
                });
    const int rc = work ? first_info(*h) : 0;
    h->last_time = tm.s();
    return rc;
  });
}

int dopt_qp_forward_reverse(dopt_handle* h, const double* dl_dz, const double* dQ,
                            const double* dq, const double* dG, const double* dh,
                            const double* dA, const double* db, double* out_rev,
                            double* out_fwd) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "dopt_qp_forward_reverse on a non-QP handle");
    if (!dl_dz || !out_rev || !out_fwd) throw Error(-1, "dl_dz, out_rev and out_fwd are required");
    Timer tm;
    const size_t B = h->batch, L = (size_t)h->n + h->m + h->p;
    const bool device = h->mem == DOPT_MEM_DEVICE;
    staged_call(*h, 1, qp_ins(*h, dl_dz, dQ, dq, dG, dh, dA, db), {{out_rev, 0, B * L}, {out_fwd, 1, B * L}},
                [&](const double** i, double** o) {
                  h->factored = false;  // one solve = factor + fwd + rev (the factors are kept for later calls)
                  if (h->sparse) {      // both LSQR runs in one launch
                    dopt::sp_forward_reverse(*h, i[0], fwd_tangents(*h, i + 1), o[0], o[1]);
                  } else {
                    h->info_clear = false;
                    dopt::qp_forward_reverse(*h, i[0], i[1], i[2], i[3], i[4], i[5], i[6], o[0], o[1]);
                  }
                });
    // device mode returns stream-ordered (the outputs land on the handle's
    // stream, i.e. the caller's): the sparse route always, the dense one with
    // every info known to be 0; else the synchronous check of the first
    // singular problem (the sparse route has no such verdict: a plain wait)
    int rc = 0;
    if (h->sparse) {
      if (!device) wait(*h);
    } else if (!(device && h->info_clear)) {
      rc = first_info(*h);
    }
    h->last_time = tm.s();
    return rc;
  });
}

// ---- `_csc` calls: sparse tangents, gradients on a pattern --------------------
// One tangent / pattern of a `_csc` call on the device: the host-side argument
// checks, then host mode copies into the handle's per-call buffers (slot k of
// spt_in / spt_val), device mode borrows.  nzval == false: a pattern.
static dopt::CscArg stage_csc(Handle& h, int k, const int64_t* cp, const int64_t* rv, const double* nz, int64_t nnz,
                              bool nzval) {
  dopt::CscArg a{nullptr, nullptr, nullptr, 0};
  if (!cp) return a;
  if (nnz < 0) throw Error(-1, "nnz must be >= 0");
  if (nnz > 0 && (!rv || (nzval && !nz))) throw Error(-1, "rowval and nzval are required when nnz > 0");
  a.cp = stage_in_i64(h, h.spt_in[2 * k], cp, (size_t)h.batch * (h.n + 1));
  a.rv = nnz ? stage_in_i64(h, h.spt_in[2 * k + 1], rv, (size_t)nnz) : nullptr;
  a.nz = nzval && nnz ? stage_in(h, h.spt_val[k], nz, (size_t)nnz) : nullptr;
  a.nnz = nnz;
  return a;
}

// the device error word of a `_csc` call's staging, cleared
static int* csc_err_clear(Handle& h) {
  h.csc_err.ensure(sizeof(int));
  DOPT_CHECK_HIP(hipMemsetAsync(h.csc_err.p, 0, sizeof(int), h.stream));
  return h.csc_err.as<int>();
}
// ... its read-back queued behind the call's work (it lands with the call's
// final wait), and raised after that wait
static void csc_err_queue(Handle& h, int* herr) {
  DOPT_CHECK_HIP(hipMemcpyAsync(herr, h.csc_err.p, sizeof(int), hipMemcpyDeviceToHost, h.stream));
}
static void csc_err_raise(int herr) {
  if (const char* msg = dopt::sp_err_message(herr)) throw Error(-1, msg);
}
static void csc_err_wait(Handle& h) {
  int herr = 0;
  csc_err_queue(h, &herr);
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));
  csc_err_raise(herr);
}

static void qp_csc_route_check(Handle& h, const char* name, const char* dense_name) {
  if (h.kind != DOPT_KIND_QP) throw Error(-1, std::string(name) + " on a non-QP handle");
  if (!h.sparse)
    throw Error(-1, std::string(name) + ": sparse-route handles only (dopt_set_sparse); a dense-route handle takes " +
                        dense_name);
  if (!h.set) throw Error(-1, std::string(name) + ": dopt_qp_set_csc has not been called");
}

int dopt_qp_forward_csc(dopt_handle* h,
                        const int64_t* dQ_colptr, const int64_t* dQ_rowval, const double* dQ_nzval, int64_t dQ_nnz,
                        const double* dq,
                        const int64_t* dG_colptr, const int64_t* dG_rowval, const double* dG_nzval, int64_t dG_nnz,
                        const double* dh,
                        const int64_t* dA_colptr, const int64_t* dA_rowval, const double* dA_nzval, int64_t dA_nnz,
                        const double* db, double* out) {
  return guarded(h, [&]() {
    qp_csc_route_check(*h, "dopt_qp_forward_csc", "dopt_qp_forward");
    if (!out) throw Error(-1, "out is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p;
    const dopt::CscArg T[3] = {stage_csc(*h, 0, dQ_colptr, dQ_rowval, dQ_nzval, dQ_nnz, true),
                               stage_csc(*h, 1, m ? dG_colptr : nullptr, dG_rowval, dG_nzval, dG_nnz, true),
                               stage_csc(*h, 2, p ? dA_colptr : nullptr, dA_rowval, dA_nzval, dA_nnz, true)};
    staged_call(*h, 1, {{dq, 2, B * n}, {m ? dh : nullptr, 4, B * m}, {p ? db : nullptr, 6, B * p}}, {{out, 1, B * L}},
                [&](const double** i, double** o) {
                  dopt::sp_forward_csc(*h, T, i[0], i[1], i[2], o[0], csc_err_clear(*h));
                });
    csc_err_wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_qp_forward_reverse_csc(dopt_handle* h, const double* dl_dz,
                                const int64_t* dQ_colptr, const int64_t* dQ_rowval, const double* dQ_nzval,
                                int64_t dQ_nnz, const double* dq,
                                const int64_t* dG_colptr, const int64_t* dG_rowval, const double* dG_nzval,
                                int64_t dG_nnz, const double* dh,
                                const int64_t* dA_colptr, const int64_t* dA_rowval, const double* dA_nzval,
                                int64_t dA_nnz, const double* db, double* out_rev, double* out_fwd) {
  return guarded(h, [&]() {
    qp_csc_route_check(*h, "dopt_qp_forward_reverse_csc", "dopt_qp_forward_reverse");
    if (!dl_dz || !out_rev || !out_fwd) throw Error(-1, "dl_dz, out_rev and out_fwd are required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p;
    const dopt::CscArg T[3] = {stage_csc(*h, 0, dQ_colptr, dQ_rowval, dQ_nzval, dQ_nnz, true),
                               stage_csc(*h, 1, m ? dG_colptr : nullptr, dG_rowval, dG_nzval, dG_nnz, true),
                               stage_csc(*h, 2, p ? dA_colptr : nullptr, dA_rowval, dA_nzval, dA_nnz, true)};
    staged_call(*h, 1, {{dl_dz, 0, B * n}, {dq, 2, B * n}, {m ? dh : nullptr, 4, B * m}, {p ? db : nullptr, 6, B * p}},
                {{out_rev, 0, B * L}, {out_fwd, 1, B * L}}, [&](const double** i, double** o) {
                  int* err = csc_err_clear(*h);
                  h->factored = false;   // as dopt_qp_forward_reverse: one solve = factor + fwd + rev
                  dopt::sp_forward_reverse_csc(*h, i[0], T, i[1], i[2], i[3], o[0], o[1], err);
                });
    csc_err_wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_qp_reverse_grads_csc(dopt_handle* h, const double* rev,
                              const int64_t* Q_colptr, const int64_t* Q_rowval, int64_t Q_nnz, double* out_dQ_nz,
                              const int64_t* G_colptr, const int64_t* G_rowval, int64_t G_nnz, double* out_dG_nz,
                              const int64_t* A_colptr, const int64_t* A_rowval, int64_t A_nnz, double* out_dA_nz) {
  return guarded(h, [&]() {
    qp_csc_route_check(*h, "dopt_qp_reverse_grads_csc", "dopt_qp_reverse_grads");
    if (!rev) throw Error(-1, "rev is required");
    const size_t B = h->batch, n = h->n, m = h->m, p = h->p, L = n + m + p;
    if (out_dQ_nz && !Q_colptr)
      throw Error(-1, "dopt_qp_reverse_grads_csc: the sparse route keeps no Q pattern; pass one");
    double* outs[3] = {out_dQ_nz, m ? out_dG_nz : nullptr, p ? out_dA_nz : nullptr};
    const dopt::CscArg P[3] = {stage_csc(*h, 0, outs[0] ? Q_colptr : nullptr, Q_rowval, nullptr, Q_nnz, false),
                               stage_csc(*h, 1, outs[1] ? G_colptr : nullptr, G_rowval, nullptr, G_nnz, false),
                               stage_csc(*h, 2, outs[2] ? A_colptr : nullptr, A_rowval, nullptr, A_nnz, false)};
    size_t cnt[3];
    for (int k = 0; k < 3; ++k) cnt[k] = !outs[k] ? 0 : P[k].cp ? (size_t)P[k].nnz : (size_t)h->sp[k - 1].nnz;
    staged_call(*h, 1, {{rev, 0, B * L}},
                {{outs[0], 0, cnt[0], true}, {outs[1], 1, cnt[1], true}, {outs[2], 2, cnt[2], true}},
                [&](const double** i, double** o) { dopt::sp_reverse_grads_at(*h, i[0], P, o, csc_err_clear(*h)); });
    csc_err_wait(*h);
    return 0;
  });
}

// ---- NonLinearProgram back-end ---------------------------------------------

int dopt_nlp_set_structure(dopt_handle* h, const int32_t* con_kind, const int8_t* has_low,
                           const int8_t* has_up, int32_t sense) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_set_structure on a non-NLP handle");
    dopt::nlp_drop_pending(*h);   // a deferred factorisation of the old inputs
    if (sense != 1 && sense != -1) throw Error(-1, "sense must be +1 (MIN_SENSE) or -1 (MAX_SENSE)");
    const int n = h->n, c = h->m;
    if (c && !con_kind) throw Error(-1, "con_kind is required when the model has constraints");
    // index maps of _compute_solution_and_bounds (nlp_utilities.jl:181-279):
    // slacks of the ≥ rows first, then of the ≤ rows, each in row order
    std::vector<int32_t> slack_of_row(c, -1), geq, leq;
    for (int k = 0; k < c; ++k) {
      if (con_kind[k] == 1) geq.push_back(k);
      else if (con_kind[k] == 2) leq.push_back(k);
      else if (con_kind[k] != 0) throw Error(-1, "con_kind entries must be 0, 1 or 2");
    }
    const int ng = (int)geq.size(), nl = (int)leq.size(), w = n + ng + nl;
    std::vector<int32_t> row_of_slack(ng + nl);
    for (int i = 0; i < ng; ++i) slack_of_row[geq[i]] = n + i, row_of_slack[i] = geq[i];
    for (int i = 0; i < nl; ++i) slack_of_row[leq[i]] = n + ng + i, row_of_slack[ng + i] = leq[i];
    std::vector<int32_t> low_idx, up_idx, lowpos(w, -1), uppos(w, -1);
    for (int j = 0; j < n; ++j)
      if (has_low && has_low[j]) low_idx.push_back(j);
    const int nlowp = (int)low_idx.size();
    for (int i = 0; i < ng; ++i) low_idx.push_back(n + i);
    for (int j = 0; j < n; ++j)
      if (has_up && has_up[j]) up_idx.push_back(j);
    const int nupp = (int)up_idx.size();
    for (int i = 0; i < nl; ++i) up_idx.push_back(n + ng + i);
    for (size_t i = 0; i < low_idx.size(); ++i) lowpos[low_idx[i]] = (int32_t)i;
    for (size_t i = 0; i < up_idx.size(); ++i) uppos[up_idx[i]] = (int32_t)i;
    std::vector<int32_t> map;
    for (auto* v : {&slack_of_row, &row_of_slack, &lowpos, &uppos, &low_idx, &up_idx})
      map.insert(map.end(), v->begin(), v->end());
    map.push_back(0);
    h->nlp_kkt = false;
    h->nlp_sense = sense;
    h->nlp_num_w = w;
    h->nlp_ng = ng;
    h->nlp_nl = nl;
    h->nlp_nlo = (int32_t)low_idx.size();
    h->nlp_nup = (int32_t)up_idx.size();
    h->nlp_nlowp = nlowp;
    h->nlp_nupp = nupp;
    h->nlp_ncons = c;
    h->nlp_rows = w + c + h->nlp_nlo + h->nlp_nup;
    dopt::nlp_configure(*h);
    h->nlp_map.ensure(map.size() * sizeof(int32_t));
    DOPT_CHECK_HIP(hipMemcpyAsync(h->nlp_map.p, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                  h->stream));
    wait(*h);
    h->nstruct = true;
    h->nset = false;
    h->nlp_spec_off = false;   // a new structure: the speculative LU launch is tried again
    return 0;
  });
}

int dopt_nlp_set(dopt_handle* h, const double* Hxx, const double* Hxp, const double* Jx,
                 const double* Jp, const double* x, const double* cval, const double* crhs,
                 const double* y, const double* xl, const double* xu, const double* yl,
                 const double* yu) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_set on a non-NLP handle");
    dopt::nlp_drop_pending(*h);   // a deferred factorisation of the old inputs
    if (!h->nstruct || h->nlp_kkt) throw Error(-1, "dopt_nlp_set: call dopt_nlp_set_structure first");
    const size_t B = h->batch, n = h->n, c = h->m, P = h->p;
    if (!Hxx || !x) throw Error(-1, "Hxx and x are required");
    if (P && !Hxp) throw Error(-1, "Hxp is required when the model has parameters");
    if (c && (!Jx || !cval || !crhs || !y)) throw Error(-1, "Jx, cval, crhs and y are required when c > 0");
    if (c && P && !Jp) throw Error(-1, "Jp is required when the model has constraints and parameters");
    if (h->nlp_nlowp && (!xl || !yl)) throw Error(-1, "xl and yl are required when a variable has a lower bound");
    if (h->nlp_nupp && (!xu || !yu)) throw Error(-1, "xu and yu are required when a variable has an upper bound");
    const double* src[12] = {Hxx, Hxp, Jx, Jp, x, cval, crhs, y, xl, xu, yl, yu};
    const size_t cnt[12] = {B * n * n, B * n * P, B * c * n, B * c * P, B * n, B * c, B * c, B * c,
                            B * n, B * n, B * n, B * n};
    for (int k = 0; k < 12; ++k) h->nin[k] = cnt[k] ? stage_in(*h, h->own_nin[k], src[k], cnt[k]) : nullptr;
    h->nset = true;
    h->nfactored = false;
    wait(*h);
    return 0;
  });
}

// dopt_nlp_set_kkt's body; `Mdev`: M already on the device (dopt_lhs_solve's
// packed copy), else M is staged as any input
static void set_kkt(Handle& h, int32_t rows, int32_t num_w, int32_t num_cons, const double* M,
                    const double* Mdev) {
  if (h.kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_set_kkt on a non-NLP handle");
  dopt::nlp_drop_pending(h);   // a deferred factorisation of the old inputs
  if (rows <= 0 || num_w < 0 || num_cons < 0 || num_w + num_cons > rows)
    throw Error(-1, "dopt_nlp_set_kkt: bad sizes");
  if (!M) throw Error(-1, "M is required");
  h.nlp_kkt = true;
  h.lhs_info.clear();   // (dopt_lhs_resolve: only after a dopt_lhs_solve of this matrix)
  h.nlp_rows = rows;
  h.nlp_num_w = num_w;
  h.nlp_ncons = num_cons;
  h.nlp_ng = h.nlp_nl = h.nlp_nlo = h.nlp_nup = h.nlp_nlowp = h.nlp_nupp = 0;
  dopt::nlp_configure(h);
  h.nlp_map.ensure(4 * sizeof(int32_t));
  for (auto& p : h.nin) p = nullptr;
  h.nin[0] = Mdev ? Mdev : stage_in(h, h.own_nin[0], M, (size_t)h.batch * rows * rows);
  h.nstruct = true;
  h.nset = true;
  h.nfactored = false;
}

int dopt_nlp_set_kkt(dopt_handle* h, int32_t rows, int32_t num_w, int32_t num_cons, const double* M) {
  return guarded(h, [&]() {
    set_kkt(*h, rows, num_w, num_cons, M, nullptr);
    wait(*h);
    return 0;
  });
}

int dopt_nlp_factor(dopt_handle* h) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_factor on a non-NLP handle");
    Timer tm;
    dopt::nlp_factor(*h, true);   // queued; the verdicts are read back by nlp_finish
    // synchronous at return unless the caller opted into the
    // deferred form (dopt_nlp_set_deferred): then the next call finishes it
    if (!h->nlp_defer) dopt::nlp_finish(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_nlp_set_deferred(dopt_handle* h, int32_t on) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_set_deferred: NLP handles only");
    if (!on && h->nlp_pending) dopt::nlp_finish(*h);   // nothing stays queued past the switch
    h->nlp_defer = on != 0;
    return 0;
  });
}

int dopt_nlp_forward(dopt_handle* h, const double* dp, double* dx, double* ddual) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_forward on a non-NLP handle");
    if (!dx || !ddual) throw Error(-1, "dx and ddual are required");
    if (h->p && !dp) throw Error(-1, "dp is required");
    Timer tm;
    const size_t B = h->batch, nd = (size_t)h->m + h->nlp_nlowp + h->nlp_nupp;
    static const double zero = 0.0;
    staged_call(*h, 1, {{h->p ? dp : nullptr, 0, B * h->p}}, {{dx, 0, B * h->n}, {ddual, 1, B * nd}},
                [&](const double** i, double** o) { dopt::nlp_forward(*h, h->p ? i[0] : &zero, o[0], o[1]); });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_nlp_reverse(dopt_handle* h, const double* dx, const double* ddual, double* dp) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_reverse on a non-NLP handle");
    if (h->p && !dp) throw Error(-1, "dp is required");
    Timer tm;
    const size_t B = h->batch, nd = (size_t)h->m + h->nlp_nlowp + h->nlp_nupp;
    staged_call(*h, 1, {{dx, 0, B * h->n}, {ddual, 1, B * nd}}, {{dp, 0, B * h->p}},
                [&](const double** i, double** o) { dopt::nlp_reverse(*h, i[0], i[1], o[0]); });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_nlp_forward_reverse(dopt_handle* h, const double* dp, const double* dx_seed, const double* ddual_seed,
                             double* dx_out, double* ddual_out, double* dp_out) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_forward_reverse on a non-NLP handle");
    if (!dx_out || !ddual_out) throw Error(-1, "dx_out and ddual_out are required");
    if (h->p && (!dp || !dp_out)) throw Error(-1, "dp and dp_out are required");
    Timer tm;
    const size_t B = h->batch, nd = (size_t)h->m + h->nlp_nlowp + h->nlp_nupp;
    static const double zero = 0.0;
    staged_call(*h, 1, {{h->p ? dp : nullptr, 0, B * h->p}, {dx_seed, 1, B * h->n}, {ddual_seed, 2, B * nd}},
                {{dx_out, 0, B * h->n}, {ddual_out, 1, B * nd}, {dp_out, 2, B * h->p}},
                [&](const double** i, double** o) {
                  dopt::nlp_forward_reverse(*h, h->p ? i[0] : &zero, i[1], i[2], o[0], o[1], o[2]);
                });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_nlp_jacobian(dopt_handle* h, double* ds) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP) throw Error(-1, "dopt_nlp_jacobian on a non-NLP handle");
    if (!ds) throw Error(-1, "ds is required");
    const size_t cnt = (size_t)h->batch * h->nlp_rows * h->p;
    staged_call(*h, 1, {}, {{ds, 0, cnt}}, [&](const double**, double** o) { dopt::nlp_jacobian(*h, o[0]); });
    wait(*h);
    return 0;
  });
}

int dopt_nlp_kkt_solve(dopt_handle* h, int32_t k, const double* rhs, double* x) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_NLP || !h->nlp_kkt) throw Error(-1, "dopt_nlp_kkt_solve needs dopt_nlp_set_kkt");
    if (k <= 0) throw Error(-1, "k must be positive");
    if (!rhs || !x) throw Error(-1, "rhs and x are required");
    const size_t cnt = (size_t)k * h->batch * h->nlp_rows;
    staged_call(*h, 1, {{rhs, 0, cnt}}, {{x, 0, cnt}},
                [&](const double** i, double** o) { dopt::nlp_kkt_solve(*h, k, i[0], o[0]); });
    wait(*h);
    return 0;
  });
}

int dopt_lhs_solve(dopt_handle* h, int32_t rows, const double* M, int32_t k, const double* rhs, double* x,
                   int32_t iterative) {
  if (!h) return -1;
  std::vector<int32_t> info(h->batch, 0);
  const int rc = guarded(h, [&]() {
    Timer tm;
    // a small host-mode system (the Julia plug point's one model): M and the
    // right-hand sides in one pinned copy, the solution back by one
    const size_t mcnt = rows > 0 ? (size_t)h->batch * rows * rows : 0;
    const size_t cnt = rows > 0 && k > 0 ? (size_t)k * h->batch * rows : 0;
    const PackIn pi[2] = {{M, mcnt * sizeof(double)}, {rhs, cnt * sizeof(double)}};
    const void* pd[2] = {nullptr, nullptr};
    const bool small = (mcnt + cnt) * sizeof(double) <= LHS_PACK_MAX && M && rhs && x && cnt &&
                       h->kind == DOPT_KIND_NLP && use_pinned(*h) && pack_in(*h, pi, 2, pd, &h->tpack);
    set_kkt(*h, rows, rows, 0, M, small ? static_cast<const double*>(pd[0]) : nullptr);
    if (k <= 0) throw Error(-1, "k must be positive");
    if (!rhs || !x) throw Error(-1, "rhs and x are required");
    if (small) {
      double* o = out_ptr(*h, h->tout[0], x, cnt);
      dopt::lhs_solve(*h, k, static_cast<const double*>(pd[1]), o, iterative != 0, info.data());
      pinned_copy_out(*h, x, o, cnt);
    } else {
      staged_call(*h, 1, {{rhs, 0, cnt}}, {{x, 0, cnt}}, [&](const double** i, double** o) {
        dopt::lhs_solve(*h, k, i[0], o[0], iterative != 0, info.data());
      });
      wait(*h);
    }
    h->last_time = tm.s();
    return 0;
  });
  if (rc) return rc;
  for (int32_t v : info)
    if (v > 0) return v;   // LHS \ RHS raises SingularException(info)
  return 0;
}

int dopt_lhs_resolve(dopt_handle* h, int32_t k, const double* rhs, double* x, int32_t trans) {
  if (!h) return -1;
  std::vector<int32_t> info(h->batch, 0);
  const int rc = guarded(h, [&]() {
    if (k <= 0) throw Error(-1, "k must be positive");
    if (!rhs || !x) throw Error(-1, "rhs and x are required");
    Timer tm;
    const size_t cnt = (size_t)k * h->batch * h->nlp_rows;
    const PackIn pi[1] = {{rhs, cnt * sizeof(double)}};
    const void* pd[1] = {nullptr};
    // (its own device buffer: tpack still holds M when dopt_lhs_solve packed it,
    // and nin[0] points there for a later re-factorisation)
    const bool small = cnt * sizeof(double) <= LHS_PACK_MAX && use_pinned(*h) && pack_in(*h, pi, 1, pd, &h->rpack);
    if (small) {   // (as dopt_lhs_solve: one pinned copy each way)
      double* o = out_ptr(*h, h->tout[0], x, cnt);
      dopt::lhs_resolve(*h, k, static_cast<const double*>(pd[0]), o, trans != 0, info.data());
      pinned_copy_out(*h, x, o, cnt);
    } else {
      staged_call(*h, 1, {{rhs, 0, cnt}}, {{x, 0, cnt}}, [&](const double** i, double** o) {
        dopt::lhs_resolve(*h, k, i[0], o[0], trans != 0, info.data());
      });
      wait(*h);
    }
    h->last_time = tm.s();
    return 0;
  });
  if (rc) return rc;
  for (int32_t v : info)
    if (v > 0) return v;
  return 0;
}

int dopt_nlp_get_corrections(dopt_handle* h, int32_t* corr) {
  return guarded(h, [&]() {
    if (!corr) throw Error(-1, "corr is required");
    if (!h->nfactored) throw Error(-1, "dopt_nlp_get_corrections: not factorised");
    dopt::nlp_finish(*h);
    std::copy(h->nlp_corr.begin(), h->nlp_corr.end(), corr);
    return 0;
  });
}

int dopt_nlp_get_layout(dopt_handle* h, int32_t* layout) {
  return guarded(h, [&]() {
    if (!layout) throw Error(-1, "layout is required");
    const int32_t v[7] = {h->nlp_rows, h->nlp_num_w, h->nlp_ncons, h->nlp_nlo, h->nlp_nup, h->nlp_nlowp,
                          h->nlp_nupp};
    std::copy(v, v + 7, layout);
    return 0;
  });
}

int dopt_get_info(dopt_handle* h, int32_t* info) {
  return guarded(h, [&]() {
    if (!info) throw Error(-1, "info is required");
    if (h->kind == DOPT_KIND_QP && h->sparse) {   // LSQR only: never singular
      std::fill(info, info + h->batch, 0);
    } else if (h->kind == DOPT_KIND_QP) {
      const std::vector<dopt::QPMeta> meta = read_meta(*h);
      for (int64_t i = 0; i < h->batch; ++i)
        info[i] = (meta[i].iterative || meta[i].info <= 0) ? 0 : full_column(*h, i, meta[i]);
    } else {
      if (!h->cinfo.p) throw Error(-1, "no conic solve has run");
      read_back(*h, info, h->cinfo.p, h->batch * sizeof(int32_t));
    }
    return 0;
  });
}

int dopt_qp_get_kept(dopt_handle* h, int8_t* kept) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "QP only");
    if (!kept) throw Error(-1, "kept is required");
    if (h->sparse) throw Error(-1, "the sparse route eliminates no rows (LSQR on the full LHS)");
    if (!h->factored && !h->small_ready) throw Error(-1, "no factorisation has run");
    const size_t B = h->batch, m = h->m;
    std::vector<int32_t> rpos(B * m);
    if (B * m)
      DOPT_CHECK_HIP(hipMemcpyAsync(rpos.data(), h->kidx.as<int32_t>() + B * m, B * m * sizeof(int32_t),
                                    hipMemcpyDeviceToHost, h->stream));
    wait(*h);
    for (size_t i = 0; i < B * m; ++i) kept[i] = rpos[i] >= 0;
    return 0;
  });
}

int dopt_qp_get_lu_kind(dopt_handle* h, int8_t* kinds) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP && h->kind != DOPT_KIND_NLP) throw Error(-1, "QP and NLP handles only");
    if (!kinds) throw Error(-1, "kinds is required");
    if (h->kind == DOPT_KIND_NLP) {
      // dopt_nlp_factor returns with the LU queued: the finish step (fallbacks,
      // inertia corrections, a missed speculative launch) sets the final kinds
      if (!h->nfactored) throw Error(-1, "no NLP factorisation has run");
      dopt::nlp_finish(*h);
    }
    if (h->sparse) {   // every problem on the LSQR branch (dopt_qp_factor refuses any other)
      std::fill(kinds, kinds + h->batch, (int8_t)DOPT_LU_KIND_LSQR);
      return 0;
    }
    const std::vector<dopt::QPMeta> meta = read_meta(*h);
    for (int64_t i = 0; i < h->batch; ++i) {
      const auto& mm = meta[i];
      const int r = dopt::qp_route(mm.iterative, mm.nsys);
      kinds[i] = r == dopt::ROUTE_LSQR ? DOPT_LU_KIND_LSQR
                 : r == dopt::ROUTE_GENERIC ? DOPT_LU_KIND_PIVOT
                 : mm.lu == dopt::LU_NOPIV ? DOPT_LU_KIND_NOPIV
                 : mm.lu == dopt::LU_SMALL ? DOPT_LU_KIND_SMALL : DOPT_LU_KIND_PIVOT;
    }
    return 0;
  });
}

int dopt_qp_get_sym(dopt_handle* h, int8_t* flags) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "QP only");
    if (!flags) throw Error(-1, "flags is required");
    if (h->sparse) {   // LSQR only: no factorisation, so no P-symmetric route (meta may be unallocated)
      std::fill(flags, flags + h->batch, (int8_t)0);
      return 0;
    }
    const std::vector<dopt::QPMeta> meta = read_meta(*h);
    for (int64_t i = 0; i < h->batch; ++i) flags[i] = meta[i].sym && meta[i].lu == dopt::LU_NOPIV ? 1 : 0;
    return 0;
  });
}

int dopt_get_iterative(dopt_handle* h, int8_t* flags) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP) throw Error(-1, "QP only");
    if (!flags) throw Error(-1, "flags is required");
    if (h->sparse) {
      if (!h->set) throw Error(-1, "no model is set");
      std::fill(flags, flags + h->batch, (int8_t)(h->sp_qnz ? 0 : 1));
      return 0;
    }
    const std::vector<dopt::QPMeta> meta = read_meta(*h);
    for (int64_t i = 0; i < h->batch; ++i) flags[i] = (int8_t)meta[i].iterative;
    return 0;
  });
}

int dopt_get_system_size(dopt_handle* h, int32_t* sizes) {
  return guarded(h, [&]() {
    if (!sizes) throw Error(-1, "sizes is required");
    if (h->kind == DOPT_KIND_QP || h->kind == DOPT_KIND_NLP) {
      if (h->kind == DOPT_KIND_NLP && !h->nfactored) throw Error(-1, "no NLP factorisation has run");
      if (h->kind == DOPT_KIND_NLP) dopt::nlp_finish(*h);
      if (h->sparse) {   // the full LHS (nothing eliminated)
        std::fill(sizes, sizes + h->batch, h->n + h->m + h->p);
        return 0;
      }
      const std::vector<dopt::QPMeta> meta = read_meta(*h);
      for (int64_t i = 0; i < h->batch; ++i) sizes[i] = meta[i].nsys;
    } else {
      if (!h->cinfo.p) throw Error(-1, "no conic solve has run");
      read_back(*h, sizes, h->cinfo.as<int32_t>() + h->batch, h->batch * sizeof(int32_t));
    }
    return 0;
  });
}

int dopt_qp_lsqr_stats(dopt_handle* h, int32_t* stats) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_QP || !h->sparse) throw Error(-1, "dopt_qp_lsqr_stats: sparse-route QP handles only");
    if (!stats) throw Error(-1, "stats is required");
    if (!h->sp_info.p) throw Error(-1, "no sparse solve has run");
    read_back(*h, stats, h->sp_info.p, 4 * h->batch * sizeof(int32_t));
    return 0;
  });
}

double dopt_last_time(const dopt_handle* h) { return h ? h->last_time : -1.0; }

int dopt_set_profiling(dopt_handle* h, int32_t on) {
  return guarded(h, [&]() {
    h->collect_phases();
    h->prof = on != 0 ? ~0u : 0u;
    return 0;
  });
}

int dopt_set_profiling_phases(dopt_handle* h, uint32_t mask) {
  return guarded(h, [&]() {
    h->collect_phases();
    h->prof = mask;
    return 0;
  });
}

int dopt_get_phase_times(dopt_handle* h, double* ms, int32_t* counts, int32_t nphases) {
  return guarded(h, [&]() {
    if (nphases < 0 || nphases > DOPT_NUM_PHASES) throw Error(-1, "bad nphases");
    h->collect_phases();
    for (int i = 0; i < nphases; ++i) {
      if (ms) ms[i] = h->phase_ms[i];
      if (counts) counts[i] = h->phase_cnt[i];
    }
    for (int i = 0; i < DOPT_NUM_PHASES; ++i) {
      h->phase_ms[i] = 0.0;
      h->phase_cnt[i] = 0;
    }
    return 0;
  });
}

const char* dopt_phase_name(int32_t phase) {
  static const char* names[DOPT_NUM_PHASES] = {
      "qp_assemble", "qp_lu", "qp_lu_pivot", "qp_rhs", "qp_solve", "qp_lsqr", "qp_output",
      "conic_cone", "conic_rhs", "conic_lsqr", "conic_output"};
  return (phase >= 0 && phase < DOPT_NUM_PHASES) ? names[phase] : "unknown";
}

// ---- conic -----------------------------------------------------------------
// cone-table validation + staging shared by the dense and CSC setters; `A` is
// already a device pointer
static void conic_set_common(Handle* h, const double* A, const double* b, const double* c,
                             const double* x, const double* s, const double* y,
                             const int32_t* cone_desc, int32_t ncones) {
  const size_t B = h->batch, n = h->n, m = h->m;
  if (!b || !c || !x || !s || !y) throw Error(-1, "A, b, c, x, s, y are required");
  if (ncones < 0 || (ncones > 0 && !cone_desc)) throw Error(-1, "bad cone table");
  int64_t rows = 0;
  for (int k = 0; k < ncones; ++k) {
    const int code = cone_desc[2 * k], dim = cone_desc[2 * k + 1];
    if (code < 0 || code > DOPT_CONE_PSD_TRI || dim < 0) throw Error(-1, "bad cone code/dimension");
    if (code == DOPT_CONE_SOC && dim < 1) throw Error(-1, "SecondOrderCone dimension must be >= 1");
    if (code == DOPT_CONE_PSD_TRI) {
      const int d = dopt::psd_side(dim);
      if (dopt::psd_tri_dim(d) != dim) throw Error(-1, "PSD triangle dimension is not triangular");
      if (d > 4096) throw Error(-1, "PSD cones larger than 4096×4096 are not supported");
    }
    rows += dim;
  }
  if (rows != (int64_t)m) throw Error(-1, "cone dimensions do not add up to m");
  h->cones.assign(cone_desc, cone_desc + 2 * ncones);
  h->cA = A;
  h->cb = stage_in(*h, h->own_cin[1], b, B * m);
  h->cc = stage_in(*h, h->own_cin[2], c, B * n);
  h->cx = stage_in(*h, h->own_cin[3], x, B * n);
  h->cs = stage_in(*h, h->own_cin[4], s, B * m);
  h->cy = stage_in(*h, h->own_cin[5], y, B * m);
  h->cset = true;
  h->cfactored = false;
  h->conic_k = 0;
  wait(*h);
}

int dopt_conic_set(dopt_handle* h, const double* A, const double* b, const double* c,
                   const double* x, const double* s, const double* y,
                   const int32_t* cone_desc, int32_t ncones) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_set on a non-conic handle");
    if (h->sparse) throw Error(-1, "dopt_conic_set: a sparse-route handle takes the MOI matrix form (dopt_conic_set_csc)");
    if (!A) throw Error(-1, "A, b, c, x, s, y are required");
    // the staging below overwrites the previous model's A before the cone
    // table is validated: the handle holds no model until this call succeeds
    h->cset = h->cfactored = false;
    conic_set_common(h, stage_in(*h, h->own_cin[0], A, (size_t)h->batch * h->m * h->n), b, c, x, s, y,
                     cone_desc, ncones);
    return 0;
  });
}

int dopt_conic_set_csc(dopt_handle* h, const int64_t* A_colptr, const int64_t* A_rowval,
                       const double* A_nzval, int64_t A_nnz, const double* b, const double* c,
                       const double* x, const double* s, const double* y,
                       const int32_t* cone_desc, int32_t ncones) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_set_csc on a non-conic handle");
    const size_t B = h->batch, n = h->n, m = h->m;
    if (!A_colptr) throw Error(-1, "A, b, c, x, s, y are required");
    if (A_nnz < 0 || (A_nnz > 0 && (!A_rowval || !A_nzval))) throw Error(-1, "bad CSC nnz / arrays");
    // A is densified (or its sparse store rebuilt) before the CSC arrays and
    // the cone table are validated: the handle holds no model until this
    // call succeeds
    h->cset = h->cfactored = false;
    h->csc_err.ensure(sizeof(int));
    DOPT_CHECK_HIP(hipMemsetAsync(h->csc_err.p, 0, sizeof(int), h->stream));
    const int64_t* cp = stage_in_i64(*h, h->csc_in[0], A_colptr, B * (n + 1));
    const int64_t* rv = stage_in_i64(*h, h->csc_in[1], A_rowval, (size_t)A_nnz);
    const double* nz = stage_in(*h, h->csc_in_val[0], A_nzval, (size_t)A_nnz);
    const double* A = nullptr;
    if (h->sparse) {   // A_moi kept sparse: CSC + its CSR copy (sparse.hip), no dense A
      // (the split LSQR applies larger sides from global scratch: dopt_create's cap of 4096 holds)
      for (int k = 0; k < ncones && cone_desc && !h->sparse_split; ++k)
        if (cone_desc[2 * k] == DOPT_CONE_PSD_TRI && cone_desc[2 * k + 1] > dopt::psd_tri_dim(64))
          throw Error(-1, "sparse conic route: PSD cones up to side 64 (their Dπ apply runs in LDS)");
      if (m) dopt::sp_stage(*h, h->sp[0], cp, rv ? rv : cp, nz, A_nnz, (int)m, h->csc_err.as<int>());
    } else {
      DevBuf& d = h->own_cin[0];
      d.ensure(std::max<size_t>(B * m * n, 1) * sizeof(double));
      if (m) dopt::csc_to_dense(*h, cp, rv ? rv : cp, nz ? nz : d.as<double>(), A_nnz, (int)m, (int)n,
                                d.as<double>(), h->csc_err.as<int>());
      A = d.as<double>();
    }
    if (const int herr = csc_err_read(*h)) throw Error(-1, csc_err_text(herr));
    conic_set_common(h, A, b, c, x, s, y, cone_desc, ncones);
    return 0;
  });
}

int dopt_conic_factor(dopt_handle* h) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_factor on a non-conic handle");
    dopt::conic_factor(*h);
    wait(*h);
    return 0;
  });
}

int dopt_conic_forward(dopt_handle* h, const double* dA, const double* db, const double* dc,
                       double* out, double* out_dx) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_forward on a non-conic handle");
    h->conic_k = 0;
    if (!out) throw Error(-1, "out is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    staged_call(*h, 1, {{dA, 1, B * m * n}, {db, 2, B * m}, {dc, 3, B * n}}, {{out, 0, B * N}, {out_dx, 1, B * n}},
                [&](const double** i, double** o) { dopt::conic_forward(*h, i[0], i[1], i[2], o[0], o[1]); });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_conic_forward_reverse(dopt_handle* h, const double* dA, const double* db, const double* dc,
                               const double* dx, double* out, double* out_dx, double* out_g, double* out_dA,
                               double* out_db, double* out_dc) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_forward_reverse on a non-conic handle");
    h->conic_k = 0;
    if (!out || !dx || !out_g) throw Error(-1, "out, dx and out_g are required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    staged_call(*h, 1, {{dA, 1, B * m * n}, {db, 2, B * m}, {dc, 3, B * n}, {dx, 0, B * n}},
               {{out, 0, B * N}, {out_dx, 1, B * n}, {out_g, 2, B * N}, {out_dA, 3, B * m * n}, {out_db, 4, B * m},
                {out_dc, 5, B * n}},
                [&](const double** i, double** o) {
                 dopt::conic_forward_reverse(*h, i[0], i[1], i[2], i[3], o[0], o[1], o[2], o[3], o[4], o[5]);
               });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_conic_set_maxiter(dopt_handle* h, int32_t maxiter) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_set_maxiter on a non-conic handle");
    if (maxiter < 0) throw Error(-1, "maxiter must be >= 0");
    h->lsqr_cap = maxiter;
    return 0;
  });
}

// (what cinfo, cnorm and cinfok hold after each kind of call: the slot table at ConicSeq, conic.hip)
int dopt_conic_lsqr_stats(dopt_handle* h, int32_t* stats) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_lsqr_stats on a non-conic handle");
    if (!stats) throw Error(-1, "stats is required");
    if (!h->cinfo.p) throw Error(-1, "no conic solve has run");
    read_back(*h, stats, h->cinfo.p, 4 * h->batch * sizeof(int32_t));
    return 0;
  });
}

int dopt_conic_lsqr_norms(dopt_handle* h, double* norms) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_lsqr_norms on a non-conic handle");
    if (!norms) throw Error(-1, "norms is required");
    if (!h->cnorm.p) throw Error(-1, "no conic solve has run");
    read_back(*h, norms, h->cnorm.p, 8 * h->batch * sizeof(double));
    return 0;
  });
}

int dopt_conic_reverse(dopt_handle* h, const double* dx, double* out_g, double* out_dA,
                       double* out_db, double* out_dc) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_reverse on a non-conic handle");
    h->conic_k = 0;
    if (!dx || !out_g) throw Error(-1, "dx and out_g are required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    staged_call(*h, 1, {{dx, 0, B * n}},
               {{out_g, 2, B * N}, {out_dA, 3, B * m * n}, {out_db, 4, B * m}, {out_dc, 5, B * n}},
                [&](const double** i, double** o) { dopt::conic_reverse(*h, i[0], o[0], o[1], o[2], o[3]); });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_conic_reverse_k(dopt_handle* h, int32_t k, const double* dx, double* out_g, double* out_dA,
                         double* out_db, double* out_dc) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_reverse_k on a non-conic handle");
    h->conic_k = 0;
    if (k < 1) throw Error(-1, "dopt_conic_reverse_k: k must be at least 1");
    if (!dx || !out_g) throw Error(-1, "dx and out_g are required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    staged_call(*h, k, {{dx, 0, B * n}},
               {{out_g, 2, B * N}, {out_dA, 3, B * m * n}, {out_db, 4, B * m}, {out_dc, 5, B * n}},
                [&](const double** i, double** o) { dopt::conic_reverse_k(*h, k, i[0], o[0], o[1], o[2], o[3]); });
    wait(*h);
    h->conic_k = k;
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_conic_forward_k(dopt_handle* h, int32_t k, const double* dA, const double* db, const double* dc,
                         double* out, double* out_dx) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_forward_k on a non-conic handle");
    h->conic_k = 0;
    if (k < 1) throw Error(-1, "dopt_conic_forward_k: k must be at least 1");
    if (!out) throw Error(-1, "out is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    staged_call(*h, k, {{dA, 1, B * m * n}, {db, 2, B * m}, {dc, 3, B * n}}, {{out, 0, B * N}, {out_dx, 1, B * n}},
                [&](const double** i, double** o) { dopt::conic_forward_k(*h, k, i[0], i[1], i[2], o[0], o[1]); });
    wait(*h);
    h->conic_k = k;
    h->last_time = tm.s();
    return 0;
  });
}

// The tangent dA of a conic `_csc` call into h.spt[0] (the staging counts as
// right-hand-side time); false: absent, the call takes the dense entry's path
// with dA == null
static bool conic_stage_tangent(Handle& h, const int64_t* cp, const int64_t* rv, const double* nz, int64_t nnz) {
  if (!h.cset) throw Error(-1, "no conic model is set (dopt_conic_set / dopt_conic_set_csc)");
  const dopt::CscArg T = stage_csc(h, 0, h.m ? cp : nullptr, rv, nz, nnz, true);
  if (!T.cp) return false;
  int* err = csc_err_clear(h);
  dopt::PhaseTimer pt(h, DOPT_PHASE_CONIC_RHS);
  dopt::sp_stage(h, h.spt[0], T.cp, T.rv ? T.rv : T.cp, T.nz, T.nnz, h.m, err, true);
  return true;
}

int dopt_conic_forward_csc(dopt_handle* h, const int64_t* dA_colptr, const int64_t* dA_rowval,
                           const double* dA_nzval, int64_t dA_nnz, const double* db, const double* dc,
                           double* out, double* out_dx) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_forward_csc on a non-conic handle");
    h->conic_k = 0;
    if (!out) throw Error(-1, "out is required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    const bool sp = conic_stage_tangent(*h, dA_colptr, dA_rowval, dA_nzval, dA_nnz);
    int herr = 0;
    staged_call(*h, 1, {{db, 2, B * m}, {dc, 3, B * n}}, {{out, 0, B * N}, {out_dx, 1, B * n}},
                [&](const double** i, double** o) {
                 if (sp) dopt::conic_forward_csc(*h, h->spt[0], h->csc_err.as<int>(), i[0], i[1], o[0], o[1]);
                 else dopt::conic_forward(*h, nullptr, i[0], i[1], o[0], o[1]);
                 if (sp) csc_err_queue(*h, &herr);
               });
    wait(*h);
    csc_err_raise(herr);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_conic_forward_reverse_csc(dopt_handle* h, const int64_t* dA_colptr, const int64_t* dA_rowval,
                                   const double* dA_nzval, int64_t dA_nnz, const double* db, const double* dc,
                                   const double* dx, double* out, double* out_dx, double* out_g,
                                   double* out_db, double* out_dc) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_forward_reverse_csc on a non-conic handle");
    h->conic_k = 0;
    if (!out || !dx || !out_g) throw Error(-1, "out, dx and out_g are required");
    Timer tm;
    const size_t B = h->batch, n = h->n, m = h->m, N = n + m + 1;
    const bool sp = conic_stage_tangent(*h, dA_colptr, dA_rowval, dA_nzval, dA_nnz);
    int herr = 0;
    staged_call(*h, 1, {{db, 2, B * m}, {dc, 3, B * n}, {dx, 0, B * n}},
               {{out, 0, B * N}, {out_dx, 1, B * n}, {out_g, 2, B * N}, {out_db, 4, B * m}, {out_dc, 5, B * n}},
                [&](const double** i, double** o) {
                 if (sp)
                   dopt::conic_forward_reverse_csc(*h, h->spt[0], h->csc_err.as<int>(), i[0], i[1], i[2], o[0], o[1],
                                                   o[2], o[3], o[4]);
                 else
                   dopt::conic_forward_reverse(*h, nullptr, i[0], i[1], i[2], o[0], o[1], o[2], nullptr, o[3], o[4]);
                 if (sp) csc_err_queue(*h, &herr);
               });
    wait(*h);
    csc_err_raise(herr);
    h->last_time = tm.s();
    return 0;
  });
}

int dopt_conic_reverse_grads_csc(dopt_handle* h, const double* g, const int64_t* P_colptr,
                                 const int64_t* P_rowval, int64_t P_nnz, double* out_nz) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_reverse_grads_csc on a non-conic handle");
    if (!g || !out_nz) throw Error(-1, "g and out_nz are required");
    const size_t B = h->batch, N = (size_t)h->n + h->m + 1;
    const dopt::CscArg P = stage_csc(*h, 0, P_colptr, P_rowval, nullptr, P_nnz, false);
    const size_t cnt = P.cp ? (size_t)P.nnz : h->sparse ? (size_t)h->sp[0].nnz : 0;   // (refusals: conic_reverse_grads_at)
    staged_call(*h, 1, {{g, 0, B * N}}, {{out_nz, 3, cnt, true}}, [&](const double** i, double** o) {
      dopt::conic_reverse_grads_at(*h, i[0], P, o[0], csc_err_clear(*h));
    });
    csc_err_wait(*h);
    return 0;
  });
}

int dopt_conic_lsqr_stats_k(dopt_handle* h, int32_t k, int32_t* stats) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_lsqr_stats_k on a non-conic handle");
    if (!stats) throw Error(-1, "stats is required");
    if (k < 1) throw Error(-1, "dopt_conic_lsqr_stats_k: k must be at least 1");
    if (h->conic_k != k || !h->cinfok.p)
      throw Error(-1, "dopt_conic_lsqr_stats_k: the last conic call was not a _k call with this k");
    read_back(*h, stats, h->cinfok.p, (size_t)2 * h->batch * k * sizeof(int32_t));
    return 0;
  });
}

// ---- conic parameter accumulation (params.hip) ----
int dopt_conic_params_forward(dopt_handle* h, const double* dp, int32_t nparam, int64_t nterms,
                              const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                              const double* t_coef, double* db, double* dc) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_params_forward on a non-conic handle");
    if ((nparam > 0 && !dp) || (h->m && !db) || (h->n && !dc))
      throw Error(-1, "dp, db (m > 0) and dc (n > 0) are required");
    const size_t B = h->batch, n = h->n, m = h->m, P = nparam > 0 ? (size_t)nparam : 0;
    staged_call(*h, 1, {{P ? dp : nullptr, 0, B * P}}, {{m ? db : nullptr, 4, B * m}, {n ? dc : nullptr, 5, B * n}},
                [&](const double** i, double** o) {
                  dopt::conic_params_forward(*h, i[0], nparam, nterms, t_param, t_kind, t_index, t_coef, o[0], o[1]);
                });
    wait(*h);
    return 0;
  });
}

int dopt_conic_params_reverse(dopt_handle* h, const double* g, int32_t nparam, int64_t nterms,
                              const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                              const double* t_coef, double* out_dp) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_params_reverse on a non-conic handle");
    if (!g || (nparam > 0 && !out_dp)) throw Error(-1, "g and out_dp are required");
    const size_t B = h->batch, N = (size_t)h->n + h->m + 1, P = nparam > 0 ? (size_t)nparam : 0;
    staged_call(*h, 1, {{g, 0, B * N}}, {{P ? out_dp : nullptr, 0, B * P}}, [&](const double** i, double** o) {
      dopt::conic_params_reverse(*h, i[0], nparam, nterms, t_param, t_kind, t_index, t_coef, o[0]);
    });
    wait(*h);
    return 0;
  });
}

int dopt_conic_params_jacobian(dopt_handle* h, int32_t mode, int32_t nparam, int64_t nterms,
                               const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                               const double* t_coef, double* out_J, int32_t* stats) {
  return guarded(h, [&]() {
    if (h->kind != DOPT_KIND_CONIC) throw Error(-1, "dopt_conic_params_jacobian on a non-conic handle");
    h->conic_k = 0;   // the chunks' _k calls are not the caller's: `stats` is the way to read the runs
    const size_t cnt = (size_t)h->batch * h->n * (nparam > 0 ? (size_t)nparam : 0);
    if (cnt && !out_J) throw Error(-1, "out_J is required");
    Timer tm;
    staged_call(*h, 1, {}, {{cnt ? out_J : nullptr, 0, cnt}}, [&](const double**, double** o) {
      dopt::conic_params_jacobian(*h, mode, nparam, nterms, t_param, t_kind, t_index, t_coef, o[0], stats);
    });
    wait(*h);
    h->last_time = tm.s();
    return 0;
  });
}

}  // extern "C"
