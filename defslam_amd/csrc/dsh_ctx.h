// Internal definition of the opaque dsh_ctx (shared by the translation units of libdefslam_hip.so) and the host-side plumbing every
// C ABI module uses: error reporting (dsh_fail, HIPCHK), the device gate (dsh_enter), scratch slices (DevBuf), block layout (Arena),
// page-locked host buffers (HostBuf), the one-copy blocks of a call (UpBlock, DownBlock), the life cycle of the device-resident
// stores (dsh_store, DSH_STORE_ENTER / DSH_STORE_GATE / DSH_CHECK, dsh_store_grow) and what the mapping calls share across files
// (namespace dsh).
//
// How a call moves its arrays.  An array of the caller whose byte count is known before the copy is a bound slice: up.copy_of(src, bytes)
// on the way up, down.copy_to(dst, bytes) on the way down; a null array or no bytes is an empty slice, and dev_if() hands the kernel null
// for it.  A call whose blocks hold bound slices alone is up.copy(c), launches, down.receive(c).  Three kinds of slice stay by hand, each
// with a one-line comment where it is filled or read:
//   - what the host computes or converts: zeroed counters, packed records (TrkProb), widened or merged flags, in_view (int32 on the
//     device, uint8 for the caller), fields of a result record;
//   - an output whose length comes down with it (local_kf, the anchor lists, slots / idx, new_idx): the caller gets exactly that many
//     entries, never the capacity that was fetched;
//   - a call that can refuse after the download (TRK_REFUSED, lists that do not fit): fetch and synchronise by hand, check, then
//     hand_out(), so a refused call leaves the caller's arrays untouched.
// A slice the kernels write whether the caller asked for it or not keeps its bytes: take() it and bind it with copy_to(off, dst, bytes).
// A DownBlock placed with at() over an array of a store ends in take_exact(): a padded last slice would read past the allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/defslam_hip.h"

// Grow-only device scratch of a context: the one-shot calls (BBS, normals, Schwarp) carve their temporaries out of it
// instead of paying a dozen hipMalloc/hipFree per call.  reset() at the start of a call, release() in dsh_destroy.
// A context serves one host thread at a time (it also owns one stream).
struct dsh_scratch {
  std::vector<std::pair<char*, size_t>> chunks;
  size_t chunk = 0, off = 0;
  void reset() { chunk = 0; off = 0; }
  hipError_t take(size_t bytes, void** out) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    for (; chunk < chunks.size(); chunk++, off = 0)
      if (off + bytes <= chunks[chunk].second) {
        *out = chunks[chunk].first + off;
        off += bytes;
        return hipSuccess;
      }
    const size_t cap = bytes > ((size_t)8 << 20) ? bytes : ((size_t)8 << 20);
    char* p = nullptr;
    const hipError_t e = hipMalloc((void**)&p, cap);
    if (e != hipSuccess) return e;
    chunks.emplace_back(p, cap);
    chunk = chunks.size() - 1;
    *out = p;
    off = bytes;
    return hipSuccess;
  }
  void release() {
    for (auto& c : chunks) (void)hipFree(c.first);
    chunks.clear();
    reset();
  }
};

// Host buffer of a context that the copy engine reads / writes directly: page-locked for a GPU context (hipMemcpyAsync
// from pageable memory is staged and synchronous), plain memory for a host-only one.  Grow-only.
struct HostBuf {
  char* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  hipError_t ensure(size_t bytes, bool want_pinned) {
    if (bytes <= cap) return hipSuccess;
    release();
    const size_t want = bytes + bytes / 4 + 4096;
    if (want_pinned) {
      const hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
      if (e != hipSuccess) { p = nullptr; return e; }
      pinned = true;
    } else {
      p = static_cast<char*>(std::malloc(want));
      if (!p) return hipErrorOutOfMemory;
      pinned = false;
    }
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (p) { if (pinned) (void)hipHostFree(p); else std::free(p); }
    p = nullptr; cap = 0;
  }
};

// Byte layout of a block that moves in one copy (or one device allocation): 256-byte aligned slices.
struct Arena {
  size_t size = 0;
  static size_t round(size_t bytes) { return (bytes + 255) & ~size_t(255); }
  size_t take(size_t bytes) {
    const size_t off = size;
    size += round(bytes);
    return off;
  }
};

struct dsh_store;

struct dsh_ctx_base {
  dsh_scratch scratch;
  HostBuf pin_in, pin_out;   // host side of the one-copy-in / one-copy-out blocks (UpBlock / DownBlock): they grow to the largest call's traffic and never shrink
  int device = 0;
  bool host_only = false;   // device == -1: template + packer only (CPU tests of the host logic)
  hipStream_t stream = nullptr;
  std::string err;
  std::vector<dsh_store*> stores;   // device-resident stores created on this context: dsh_destroy detaches them (dsh_detach_stores)
};
dsh_ctx_base* dsh_base(dsh_ctx* ctx);   // the opaque handle of the ABI as its base (dsh_api.cpp; dsh_ctx is complete in dsh_sft_ctx.h)
namespace dsh { struct TemplateHost; }
// the context's current template when it was built from facets, else null (a store call that embeds reaches it through its context)
const dsh::TemplateHost* dsh_facet_template(dsh_ctx_base* c);

// What the device-resident stores (dsh_diffdb, dsh_kfdb) share: the owning context and the device of their allocations.  A store works
// in either order with dsh_destroy of its context: dsh_destroy detaches it (every call on it but its destroy then returns DSH_ERR_ARG),
// and destroying it needs nothing of the context.
struct dsh_store {
  dsh_ctx_base* ctx = nullptr;   // the owning context; null after dsh_destroy of that context
  int device = 0;                // HIP device of the allocations
};
inline void dsh_attach_store(dsh_ctx_base* c, dsh_store* s) {
  s->ctx = c;
  s->device = c->device;
  c->stores.push_back(s);
}
inline void dsh_detach_stores(dsh_ctx_base* c) {
  for (dsh_store* s : c->stores) s->ctx = nullptr;
  c->stores.clear();
}
// First half of a store's destroy: wait for the whole device (the context's stream may be gone), unregister.  The store frees its arrays.
inline void dsh_store_unregister(dsh_store* s) {
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();
  if (s->ctx) {
    auto& v = s->ctx->stores;
    v.erase(std::remove(v.begin(), v.end(), s), v.end());
  }
}
// Grow-by-copy of a store's device allocation *p: a new allocation of `bytes`, then -- with nothing of the device still reading or
// writing the old one -- copy(new) moves the stored part device to device, and the old allocation is freed.  *p is unchanged on failure.
template <class Copy>
hipError_t dsh_store_grow(void** p, size_t bytes, Copy copy) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return e;
  (void)hipDeviceSynchronize();
  e = copy(static_cast<char*>(q));
  if (e != hipSuccess) { (void)hipFree(q); return e; }
  if (*p) (void)hipFree(*p);
  *p = q;
  return hipSuccess;
}
// the usual case: a device array of T grows to `cap` elements and keeps its `used` leading ones
template <class T>
hipError_t dsh_store_grow_array(T** p, size_t used, size_t cap) {
  return dsh_store_grow((void**)p, sizeof(T) * cap, [&](char* q) { return used ? hipMemcpy(q, *p, sizeof(T) * used, hipMemcpyDeviceToDevice) : hipSuccess; });
}

// error helper usable from every translation unit
inline int dsh_fail(dsh_ctx_base* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}

// A failed HIP call: drain the context's stream first (the append calls of the stores still copy from local host buffers), then DSH_ERR_HIP.
inline int dsh_fail_hip(dsh_ctx_base* c, hipError_t e, const char* call) {
  if (c && !c->host_only && c->stream) (void)hipStreamSynchronize(c->stream);
  return dsh_fail(c, DSH_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e));
}
#define HIPCHK(c, call)                                           \
  do {                                                            \
    const hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return dsh_fail_hip(c, e__, #call);    \
  } while (0)

// The gate of an entry point that needs the device; it sits where the entry point's host-only check belongs in its order of checks.
// A host-only context is DSH_ERR_NO_DEVICE (there is no CPU fallback); then the context's device is made current and its scratch reset.
inline int dsh_enter(dsh_ctx_base* c, const char* who) {
  if (!c) return DSH_ERR_ARG;
  if (c->host_only) return dsh_fail(c, DSH_ERR_NO_DEVICE, std::string(who) + ": host-only context, no GPU (there is no CPU fallback)");
  if (hipSetDevice(c->device) != hipSuccess) return dsh_fail(c, DSH_ERR_HIP, std::string(who) + ": hipSetDevice failed");
  c->scratch.reset();   // temporaries of this call come out of the context's scratch
  return DSH_OK;
}

// A slice of the context's scratch: nothing to free.
struct DevBuf {
  void* p = nullptr;
  hipError_t alloc(dsh_ctx_base* c, size_t bytes) { return c->scratch.take(bytes, &p); }
  template <class T> T* as() { return static_cast<T*>(p); }
};
// The same for a typed pointer of a kernel's argument struct: n elements.
template <class T>
hipError_t dsh_scratch_array(dsh_ctx_base* c, T** p, size_t n) { return c->scratch.take(sizeof(T) * n, (void**)p); }

// A block of a call that moves in one copy: slices laid out as by Arena, the host side in a page-locked buffer of the context, the device
// side in one scratch slice.  An empty block enqueues no copy; a take(0) slice is legal and never dereferenced.
// pin_in and pin_out are one buffer each, and HostBuf::ensure frees the old buffer when it grows: between two synchronisations of the stream
// a call stages at most one UpBlock and fetches at most one DownBlock, and reads nothing of a block's host side once the next one is staged.
struct CopyBlock : Arena {   // size: what the copy moves
  char *h = nullptr, *d = nullptr;
  // a slice without padding: the last one of a block whose copy ends with it
  size_t take_exact(size_t bytes) {
    const size_t off = size;
    size += bytes;
    return off;
  }
  template <class T> T* host(size_t off) const { return reinterpret_cast<T*>(h + off); }
  template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(d + off); }
  // the device side of a slice whose caller's array p is optional: null for an output or an input nobody passed
  template <class T> T* dev_if(const void* p, size_t off) const { return p ? dev<T>(off) : nullptr; }
  // slices that are plain copies of arrays of the caller (UpBlock::copy_of, DownBlock::copy_to): the block moves them itself; a null array
  // or one without bytes is an empty slice
  struct Bound { size_t off, bytes; void* p; };
  std::vector<Bound> bound;
  size_t bind(void* p, size_t bytes) {
    const size_t off = take(p ? bytes : 0);
    bind_at(off, p, bytes);
    return off;
  }
  // the same for a slice laid out by take() / take_exact(): one that keeps its bytes when the array is null because the kernels write it
  // in any case, or the unpadded last slice of a block that lies over an array of a store
  void bind_at(size_t off, void* p, size_t bytes) {
    if (p && bytes) bound.push_back({off, bytes, p});
  }
};

// Up: filled in pin_in after stage(), copied by send().  The two are apart because some calls stage here and copy into a store's own
// arrays.  The kernels may write the device side (counters that go up as zeros).
struct UpBlock : CopyBlock {
  // tail: bytes staged behind the block in the same page-locked buffer, at host<T>(size); they are not part of `size` and send() does
  // not move them: the caller copies them where they belong (the Schwarp fits' start values go into the head of their output block)
  int stage(dsh_ctx_base* c, size_t tail = 0) {
    HIPCHK(c, c->pin_in.ensure(size + tail, true));
    h = c->pin_in.p;
    for (const Bound& b : bound) std::memcpy(h + b.off, b.p, b.bytes);
    return DSH_OK;
  }
  // a slice that stage() fills from src
  size_t copy_of(const void* src, size_t bytes) { return bind(const_cast<void*>(src), bytes); }
  // the same at `off` of a slice laid out by hand, also for a part of one (a problem's share of a batch's slice); once the block is staged
  // the bytes are copied at once
  void copy_of(size_t off, const void* src, size_t bytes) {
    if (h && src && bytes) std::memcpy(h + off, src, bytes);
    else bind_at(off, const_cast<void*>(src), bytes);
  }
  // stage and send in one: for a block that holds bound slices alone
  int copy(dsh_ctx_base* c) {
    if (const int rc = stage(c)) return rc;
    return send(c);
  }
  // the device side ahead of send(): for a block whose records hold device addresses of its own slices
  int place(dsh_ctx_base* c) {
    HIPCHK(c, c->scratch.take(size, (void**)&d));
    return DSH_OK;
  }
  int send(dsh_ctx_base* c) {
    if (!d) {
      if (const int rc = place(c)) return rc;
    }
    if (size > 0) HIPCHK(c, hipMemcpyAsync(d, h, size, hipMemcpyHostToDevice, c->stream));
    return DSH_OK;
  }
};

// Down: the kernels write a scratch slice (alloc) or the block lies where a kernel's output is already (at: counters inside the upload
// block); fetch() copies into pin_out and does not synchronise: host() is read after the caller's hipStreamSynchronize.
struct DownBlock : CopyBlock {
  int alloc(dsh_ctx_base* c) {
    HIPCHK(c, c->scratch.take(size, (void**)&d));
    return at(c, d);
  }
  int at(dsh_ctx_base* c, void* dev_block) {
    HIPCHK(c, c->pin_out.ensure(size, true));
    h = c->pin_out.p;
    d = static_cast<char*>(dev_block);
    return DSH_OK;
  }
  int fetch(dsh_ctx_base* c) {
    if (size > 0) HIPCHK(c, hipMemcpyAsync(h, d, size, hipMemcpyDeviceToHost, c->stream));
    return DSH_OK;
  }
  // a slice that hand_out() copies to dst after the caller's hipStreamSynchronize (null: an optional output nobody asked for)
  size_t copy_to(void* dst, size_t bytes) { return bind(dst, bytes); }
  void copy_to(size_t off, void* dst, size_t bytes) { bind_at(off, dst, bytes); }
  void hand_out() const {
    for (const Bound& b : bound) std::memcpy(b.p, h + b.off, b.bytes);
  }
  // the end of a call: fetch, wait for the stream, hand out
  int receive(dsh_ctx_base* c) {
    if (const int rc = fetch(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hand_out();
    return DSH_OK;
  }
};

// The first checks of every entry point on a device-resident store `db`: a store that is alive and attached.  Leaves its context in c,
// the entry point's name (spelled here and nowhere else in its body) and two refusals with "who: message": bad(message) is DSH_ERR_ARG,
// refuse(code, message) any other code.
#define DSH_STORE_ENTER(who)                                                                  \
  if (!db || !db->ctx) return DSH_ERR_ARG;                                                    \
  [[maybe_unused]] dsh_ctx_base* c = db->ctx;                                                 \
  [[maybe_unused]] const char* const who__ = (who);                                           \
  [[maybe_unused]] auto refuse = [&](int code, const std::string& m) { return dsh_fail(c, code, std::string(who__) + ": " + m); }; \
  [[maybe_unused]] auto bad = [&](const std::string& m) { return refuse(DSH_ERR_ARG, m); }
// The device gate (dsh_enter) of that entry point, under the same name: it stays where the host-only check belongs in the order of checks.
#define DSH_STORE_GATE() \
  if (const int rc__ = dsh_enter(c, who__)) return rc__
// A validator that returns what is wrong as a std::string ("": nothing) or as a const char* (null: nothing): refuse with it through bad().
inline std::string dsh_check_text(std::string e) { return e; }
inline std::string dsh_check_text(const char* e) { return e ? e : ""; }
#define DSH_CHECK(expr)                               \
  do {                                                \
    const std::string e__ = dsh_check_text(expr);     \
    if (!e__.empty()) return bad(e__);                \
  } while (0)

// The key point count of a frame or a keyframe: what is wrong with it, or null.
inline const char* dsh_keypoint_count_error(long long N) { return N < 0 || N > (1 << 20) ? "N outside 0 .. 2^20" : nullptr; }

namespace dsh {
// Dense bending matrix of a B-spline (dsh_sfn.cpp; the warp initialisation of dsh_schwarp.cpp uses it too).
void bbs_bending_dense(const dsh_bbs* b, double lambda, double* Bm);

// Host logic of the mapping calls that writes straight into slices of an upload block; plain functions over host pointers.
// dsh_nrsfm.cpp: owner[r] = the point of record r, soa[18][R] = the transposed DiffProp records.
void normals_fill_records(int P, const int32_t* rec_ptr, const dsh_diffprop* recs, int32_t* owner, float* soa);
// dsh_sfn.cpp: the constant rows of the stacked system, tail[(N + 1) * N] = bending block and row of ones, b[2n + N + 1] = right-hand
// side (zero except N * mean_depth in the last row), ones[N].
void sfn_fill_constant_rows(const dsh_bbs* bbs, int n, double bending_weight, double mean_depth, double* tail, double* b, double* ones);
// dsh_register.cpp: which points of scaleMinMedian are candidates and where their draws start in the stream u[nu]
// (GroundTruthCalculator.cc:64-84).  cand / off: room for n entries, or both null to count.  Returns the number of candidates, -1 if the
// stream is too short; *consumed: the draws the reference makes.
int smm_walk_candidates(int n, const double* u, int64_t nu, int32_t* cand, int64_t* off, int64_t* consumed);

// The normals stage of dsh_normals_estimate and dsh_normals_estimate_db (dsh_nrsfm.cpp): work space, clears, nrsfm_launch_normals, one
// block down, the synchronise, the caller's arrays.  in: device arrays; out: host arrays, an optional one that is null gets no slice.
struct NormalsIn {
  const int32_t *rec_ptr, *owner;
  const float* soa;
  const uint8_t* is_ref;
  const float* first_n;
  const uint8_t* has_first_n;
  const float* x0;
  const uint8_t* has_x0;
  const float* ref_uv;
  const int32_t* rec_list[3];   // the database route's per-record lists on the device (point, tag, idx2): copied into the block
  float* keep_normals;          // device, [3P | 3R] or null: the normals stay behind here
};
struct NormalsOut {
  double *k1k2, *cov;
  int32_t* status;
  float* normal_ref;
  int32_t* iters;
  float* normal_rec;
  uint8_t* rec_written;
  int32_t* rec_list[3];
};
int normals_stage(dsh_ctx_base* c, int P, int R, const NormalsIn& in, const NormalsOut& out);

// dsh_tmplswitch.cpp: the body of dsh_surface_vertices behind its checks and its device gate; ctrl_dev: the depth spline on the device
// (dsh_keyframe_surface_vertices), or null for grid->depth_ctrl.
int surface_vertices_run(dsh_ctx_base* c, const dsh_surface_grid* grid, const double* ctrl_dev, double* nodes_xyz);
}  // namespace dsh
