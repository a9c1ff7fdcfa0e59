// The multi-GPU modes of the SfT solver on the C ABI (include/defslam_hip.h): the RCCL communicator (dsh_comm_*), the shared-camera
// mode (dsh_sft_shared_solve*) and the connected-mesh mode (dsh_sft_connected_solve*).  Host loops around the phase kernels of
// sft_kernels.hip (sft_sc_kernel, sft_cn_kernel); the rank's problem is uploaded and downloaded by dsh_api.cpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <dlfcn.h>

#include <memory>
#include <string>
#include <vector>

#include "dsh_sft_ctx.h"

extern "C" {

// ---- shared-camera mode across GPUs -------------------------------------------------------------------------------------
// RCCL is bound at run time (dlopen): a process that never creates a communicator does not load it, and a host process that
// already carries an RCCL (PyTorch) keeps a single copy.
namespace {
struct RcclUniqueId { char internal[128]; };
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(RcclUniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool load(std::string& err) {
    if (lib) return true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) { err = std::string("RCCL not found: ") + dlerror(); return false; }
    GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(lib, "ncclAllReduce"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!GetUniqueId || !CommInitRank || !AllReduce || !CommDestroy) { err = "RCCL symbols missing"; lib = nullptr; return false; }
    return true;
  }
};
Rccl g_rccl;
constexpr int kNcclDouble = 8, kNcclSum = 0;   // ncclFloat64, ncclSum (rccl.h)
}  // namespace

struct dsh_comm {
  int nranks = 1, rank = 0;
  void* comm = nullptr;      // ncclComm_t
  dsh_ctx* ctx = nullptr;
};

namespace {

// One rank of a shared-camera solve as the driver sees it.
struct ScRank { dsh_ctx* c; };

// The all-reduce of the exchange vectors: RCCL between processes (one local rank), or a summation kernel between the
// contexts of an in-process group.
struct ScReducer {
  dsh_comm* comm = nullptr;            // RCCL
  SftSc** d_ptrs = nullptr;            // in-process group: device array of the ranks' state pointers
  int reduce(std::vector<ScRank>& R, std::string& err) {
    if (comm) {
      dsh_ctx* c = R[0].c;
      const int rc = g_rccl.AllReduce(c->d_sc->send, c->d_sc->recv, SFT_SC_XCHG, kNcclDouble, kNcclSum, comm->comm, c->stream);
      if (rc != 0) { err = std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"); return DSH_ERR_HIP; }
      return DSH_OK;
    }
    for (auto& r : R)
      if (hipStreamSynchronize(r.c->stream) != hipSuccess) { err = "stream synchronise failed"; return DSH_ERR_HIP; }
    if (sft_sc_local_reduce(d_ptrs, (int)R.size(), R[0].c->stream) != hipSuccess || hipStreamSynchronize(R[0].c->stream) != hipSuccess) { err = "local reduce failed"; return DSH_ERR_HIP; }
    return DSH_OK;
  }
};

int sc_phase(std::vector<ScRank>& R, int phase, std::string& err) {
  for (auto& r : R) {
    dsh_ctx* c = r.c;
    (void)hipSetDevice(c->device);
    LDS_LOCK();
    if (sft_sc_launch(c->d_probs, c->d_sc, 1, phase, c->plan.max_kd, c->plan.jl_doubles, &LDS_MARKS(c).sc, c->stream) != hipSuccess) { err = "phase kernel launch failed"; return DSH_ERR_HIP; }
  }
  return DSH_OK;
}

// The Levenberg-Marquardt loop of the shared-camera mode: four phase kernels per damping trial, an all-reduce of SFT_SC_XCHG
// doubles behind LIN, FAC and SOL (sft_kernels.hip: sft_sc_kernel).  Every rank reads the same all-reduced numbers and takes
// the same decisions; the host only reads "again" / "done" of its first local rank.
int sc_solve(std::vector<ScRank>& R, ScReducer& red, int rank0, int nranks, const dsh_sft_frame* frames, dsh_sft_result* results, std::string& err) {
  const int G = (int)R.size();
  if (nranks > SFT_SC_XCHG - 13) { err = "too many ranks for the exchange vector"; return DSH_ERR_ARG; }   // (the same verdict on every rank)
  // A failure that only THIS rank sees (a bad frame, a template the mode cannot take, no memory) must not leave the other ranks inside a
  // collective: it is carried through the first all-reduce (slot 2 of the exchange vector) and every rank returns together.
  int local_rc = DSH_OK;
  std::string local_err;
  for (int g = 0; g < G; g++) {
    dsh_ctx* c = R[g].c;
    if (c->host_only) { err = "host-only context, no GPU (there is no CPU fallback)"; return DSH_ERR_NO_DEVICE; }
    (void)hipSetDevice(c->device);
    if (!c->d_sc && hipMalloc((void**)&c->d_sc, sizeof(SftSc)) != hipSuccess) { err = "out of device memory"; return DSH_ERR_HIP; }   // (nothing to exchange with)
    SftSc init{};
    init.rank = rank0 + g;
    init.nranks = nranks;
    int rc = frames[g].max_iters < 1 ? DSH_ERR_ARG : DSH_OK;
    if (rc != DSH_OK && local_rc == DSH_OK) { local_rc = rc; local_err = "max_iters must be >= 1"; }
    if (rc == DSH_OK) {
      rc = dsh_sft_upload(c, 1, &frames[g], SftUploadMode::shared_camera);
      if (rc != DSH_OK && local_rc == DSH_OK) { local_rc = rc; local_err = c->err; }
    }
    if (rc == DSH_OK && c->plan.prob[0].tile_mode != 1) {
      rc = DSH_ERR_ARG;
      if (local_rc == DSH_OK) { local_rc = rc; local_err = "the shared-camera mode needs a template with half-bandwidth <= 128 (register-window solver); dsh_sft_connected_solve takes wider ones"; }
    }
    if (rc == DSH_OK) {
      init.send[0] = (double)c->packed[0].h.nA;     // the regulariser weights divide by the JOINT counts (DefOptimizer.cc:458,497)
      init.send[1] = (double)c->packed[0].h.Es;
    }
    init.send[2] = rc == DSH_OK ? 0.0 : 1.0;
    if (hipMemcpyAsync(c->d_sc, &init, sizeof(SftSc), hipMemcpyHostToDevice, c->stream) != hipSuccess) { err = "state upload failed"; return DSH_ERR_HIP; }
  }
  int rc = red.reduce(R, err);
  if (rc != DSH_OK) return rc;
  {
    double tot3[3];
    dsh_ctx* c = R[0].c;
    if (hipMemcpyAsync(tot3, c->d_sc->recv, sizeof(tot3), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { err = "read-back failed"; return DSH_ERR_HIP; }
    if (tot3[2] != 0.0) {   // some rank could not set its patch up: every rank leaves here
      if (local_rc != DSH_OK) { err = local_err; return local_rc; }
      err = "another rank failed to set its patch up";
      return DSH_ERR_STATE;
    }
  }
  for (int g = 0; g < G; g++) {   // joint counts -> weights of every rank's problem record
    dsh_ctx* c = R[g].c;
    double tot[2];
    if (hipMemcpyAsync(tot, c->d_sc->recv, sizeof(tot), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { err = "read-back failed"; return DSH_ERR_HIP; }
    SftDev& h = c->h_probs[0];
    h.w_curv = frames[g].reg_lap / tot[0];
    h.w_str = tot[1] > 0 ? frames[g].reg_inex / tot[1] : 0.0;
    if (hipMemcpyAsync(c->d_probs, &h, sizeof(SftDev), hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { err = "problem record upload failed"; return DSH_ERR_HIP; }
  }
  for (int guard = 0; guard < DSH_MAX_ITERS + 1; guard++) {
    if ((rc = sc_phase(R, SFT_SC_LIN, err)) != DSH_OK || (rc = red.reduce(R, err)) != DSH_OK) return rc;
    int again = 0, done = 0;
    do {
      if ((rc = sc_phase(R, SFT_SC_FAC, err)) != DSH_OK || (rc = red.reduce(R, err)) != DSH_OK) return rc;
      if ((rc = sc_phase(R, SFT_SC_SOL, err)) != DSH_OK || (rc = red.reduce(R, err)) != DSH_OK) return rc;
      if ((rc = sc_phase(R, SFT_SC_CTL, err)) != DSH_OK) return rc;
      int32_t flags[2];
      dsh_ctx* c = R[0].c;
      if (hipMemcpyAsync(flags, &c->d_sc->again, sizeof(flags), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { err = "flag read-back failed"; return DSH_ERR_HIP; }
      again = flags[0];
      done = flags[1];
    } while (again);
    if (done) break;
  }
  for (int g = 0; g < G; g++) {
    R[g].c->ran = true;
    rc = dsh_sft_batch_download(R[g].c, 1, &results[g]);
    if (rc != DSH_OK) { err = R[g].c->err; return rc; }
  }
  return DSH_OK;
}

}  // namespace

int dsh_comm_unique_id(void* id) {
  std::string err;
  if (!id || !g_rccl.load(err)) return DSH_ERR_HIP;
  return g_rccl.GetUniqueId(static_cast<RcclUniqueId*>(id)) == 0 ? DSH_OK : DSH_ERR_HIP;
}

int dsh_comm_create(dsh_ctx* c, int nranks, int rank, const void* id, dsh_comm** out) {
  if (!c || !out || !id || nranks < 1 || rank < 0 || rank >= nranks) return dsh_fail(c, DSH_ERR_ARG, "dsh_comm_create: bad argument");
  *out = nullptr;
  if (const int rc = dsh_enter(c, "dsh_comm_create")) return rc;
  std::string err;
  if (!g_rccl.load(err)) return dsh_fail(c, DSH_ERR_HIP, "dsh_comm_create: " + err);
  RcclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  std::unique_ptr<dsh_comm> cm(new dsh_comm());
  cm->nranks = nranks; cm->rank = rank; cm->ctx = c;
  const int rc = g_rccl.CommInitRank(&cm->comm, nranks, uid, rank);
  if (rc != 0) return dsh_fail(c, DSH_ERR_HIP, std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"));
  *out = cm.release();
  return DSH_OK;
}

int dsh_comm_destroy(dsh_comm* cm) {
  if (!cm) return DSH_ERR_ARG;
  if (cm->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(cm->comm);
  delete cm;
  return DSH_OK;
}

int dsh_sft_shared_solve(dsh_ctx* c, dsh_comm* cm, const dsh_sft_frame* frame, dsh_sft_result* result) {
  if (!c || !cm || !frame || !result || cm->ctx != c) return dsh_fail(c, DSH_ERR_ARG, "dsh_sft_shared_solve: bad argument");
  std::vector<ScRank> R{ScRank{c}};
  ScReducer red;
  red.comm = cm;
  std::string err;
  const int rc = sc_solve(R, red, cm->rank, cm->nranks, frame, result, err);
  return rc == DSH_OK ? rc : dsh_fail(c, rc, "dsh_sft_shared_solve: " + err);
}

int dsh_sft_shared_solve_group(int G, dsh_ctx* const* ctxs, const dsh_sft_frame* frames, dsh_sft_result* results) {
  if (G < 1 || !ctxs || !frames || !results) return DSH_ERR_ARG;
  for (int g = 0; g < G; g++)
    if (!ctxs[g]) return DSH_ERR_ARG;
  dsh_ctx* c0 = ctxs[0];
  std::vector<ScRank> R;
  for (int g = 0; g < G; g++) R.push_back(ScRank{ctxs[g]});
  for (int g = 0; g < G; g++) {   // the state blocks must exist before their addresses are collected
    if (ctxs[g]->host_only) return dsh_fail(c0, DSH_ERR_NO_DEVICE, "dsh_sft_shared_solve_group: host-only context, no GPU (there is no CPU fallback)");
    (void)hipSetDevice(ctxs[g]->device);
    if (!ctxs[g]->d_sc && hipMalloc((void**)&ctxs[g]->d_sc, sizeof(SftSc)) != hipSuccess) return dsh_fail(c0, DSH_ERR_HIP, "dsh_sft_shared_solve_group: out of device memory");
  }
  std::vector<SftSc*> ptrs;
  for (int g = 0; g < G; g++) ptrs.push_back(ctxs[g]->d_sc);
  ScReducer red;
  (void)hipSetDevice(c0->device);
  if (hipMalloc((void**)&red.d_ptrs, sizeof(SftSc*) * G) != hipSuccess) return dsh_fail(c0, DSH_ERR_HIP, "dsh_sft_shared_solve_group: out of device memory");
  int rc = DSH_OK;
  std::string err;
  if (hipMemcpy(red.d_ptrs, ptrs.data(), sizeof(SftSc*) * G, hipMemcpyHostToDevice) != hipSuccess) { rc = DSH_ERR_HIP; err = "pointer table upload failed"; }
  if (rc == DSH_OK) rc = sc_solve(R, red, 0, G, frames, results, err);
  (void)hipFree(red.d_ptrs);
  return rc == DSH_OK ? rc : dsh_fail(c0, rc, "dsh_sft_shared_solve_group: " + err);
}


// ---- connected-mesh mode: one problem, one connected template, the factorisation cut in two (sft_kernels.hip: sft_cn_kernel) ----------
namespace {

// all-reduce (sum) of n doubles: send -> recv on every rank.  RCCL between two processes, a summation kernel between two contexts of one process.
int cn_allreduce(std::vector<ScRank>& R, dsh_comm* comm, double* const* send, double* const* recv, int n, std::string& err) {
  if (comm) {
    dsh_ctx* c = R[0].c;
    const int rc = g_rccl.AllReduce(send[0], recv[0], (size_t)n, kNcclDouble, kNcclSum, comm->comm, c->stream);
    if (rc != 0) { err = std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"); return DSH_ERR_HIP; }
    return DSH_OK;
  }
  for (auto& r : R)
    if (hipStreamSynchronize(r.c->stream) != hipSuccess) { err = "stream synchronise failed"; return DSH_ERR_HIP; }
  if (sft_vec_sum2(send[0], send[1], recv[0], recv[1], n, R[0].c->stream) != hipSuccess || hipStreamSynchronize(R[0].c->stream) != hipSuccess) { err = "local reduce failed"; return DSH_ERR_HIP; }
  return DSH_OK;
}

int cn_phase(std::vector<ScRank>& R, int phase, std::string& err) {
  for (auto& r : R) {
    dsh_ctx* c = r.c;
    (void)hipSetDevice(c->device);
    LDS_LOCK();
    if (sft_cn_launch(c->d_probs, c->d_sc, phase, c->plan.max_kd, c->plan.jl_doubles, &LDS_MARKS(c).cn, c->stream) != hipSuccess) { err = "phase kernel launch failed"; return DSH_ERR_HIP; }
  }
  return DSH_OK;
}

// R: the local ranks (one with RCCL, two in the in-process group); every rank packs the SAME frame.
int cn_solve(std::vector<ScRank>& R, dsh_comm* comm, int rank0, const dsh_sft_frame* frame, dsh_sft_result* results, std::string& err) {
  const int G = (int)R.size();
  int local_rc = DSH_OK;
  std::string local_err;
  for (int g = 0; g < G; g++) {
    dsh_ctx* c = R[g].c;
    if (c->host_only) { err = "host-only context, no GPU (there is no CPU fallback)"; return DSH_ERR_NO_DEVICE; }
    (void)hipSetDevice(c->device);
    if (!c->d_sc && hipMalloc((void**)&c->d_sc, sizeof(SftSc)) != hipSuccess) { err = "out of device memory"; return DSH_ERR_HIP; }
    int rc = frame->max_iters < 1 ? DSH_ERR_ARG : DSH_OK;
    if (rc != DSH_OK && local_rc == DSH_OK) { local_rc = rc; local_err = "max_iters must be >= 1"; }
    if (rc == DSH_OK) {
      rc = dsh_sft_upload(c, 1, frame, SftUploadMode::connected);
      if (rc != DSH_OK && local_rc == DSH_OK) { local_rc = rc; local_err = c->err; }
    }
    if (rc == DSH_OK && !c->plan.prob[0].split) {
      rc = DSH_ERR_ARG;
      if (local_rc == DSH_OK) { local_rc = rc; local_err = "the connected-mesh mode needs a band of at most 256 that is long enough to cut (two parts of four tile columns next to a separator of one bandwidth)"; }
    }
    SftSc init{};
    init.rank = rank0 + g;
    init.nranks = 2;
    init.send[0] = rc == DSH_OK ? 0.0 : 1.0;
    if (hipMemcpyAsync(c->d_sc, &init, sizeof(SftSc), hipMemcpyHostToDevice, c->stream) != hipSuccess) { err = "state upload failed"; return DSH_ERR_HIP; }
  }
  // rank-local failures are agreed on before the first phase (nobody is left inside a collective)
  {
    double* snd[2]; double* rcv[2];
    for (int g = 0; g < G; g++) { snd[g] = R[g].c->d_sc->send; rcv[g] = R[g].c->d_sc->recv; }
    int rc = cn_allreduce(R, comm, snd, rcv, 4, err);
    if (rc != DSH_OK) return rc;
    double bad = 0.0;
    dsh_ctx* c = R[0].c;
    if (hipMemcpyAsync(&bad, c->d_sc->recv, sizeof(bad), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { err = "read-back failed"; return DSH_ERR_HIP; }
    if (bad != 0.0) {
      if (local_rc != DSH_OK) { err = local_err; return local_rc; }
      err = "the other rank failed to set the problem up";
      return DSH_ERR_STATE;
    }
  }
  int rc;
  double* xs[2]; double* xr[2]; double* vx[2];
  int xl = 0, nx = 0;
  for (int g = 0; g < G; g++) {
    const SftDev& h = R[g].c->h_probs[0];
    xs[g] = h.part[rank0 + g].xchg; xr[g] = h.part[2].xchg; vx[g] = h.x;
    xl = h.sp_xl;
    nx = ((h.Dn + kNB - 1) / kNB) * kNB + 6;
  }
  for (int guard = 0; guard < DSH_MAX_ITERS + 1; guard++) {
    if ((rc = cn_phase(R, SFT_CN_LIN, err)) != DSH_OK) return rc;
    int again = 0, done = 0;
    do {
      if ((rc = cn_phase(R, SFT_CN_FAC, err)) != DSH_OK || (rc = cn_allreduce(R, comm, xs, xr, xl, err)) != DSH_OK) return rc;
      if ((rc = cn_phase(R, SFT_CN_SOL, err)) != DSH_OK || (rc = cn_allreduce(R, comm, vx, vx, nx, err)) != DSH_OK) return rc;
      if ((rc = cn_phase(R, SFT_CN_CTL, err)) != DSH_OK) return rc;
      int32_t flags[2];
      dsh_ctx* c = R[0].c;
      if (hipMemcpyAsync(flags, &c->d_sc->again, sizeof(flags), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { err = "flag read-back failed"; return DSH_ERR_HIP; }
      again = flags[0];
      done = flags[1];
    } while (again);
    if (done) break;
  }
  for (int g = 0; g < G; g++) {
    R[g].c->ran = true;
    rc = dsh_sft_batch_download(R[g].c, 1, &results[g]);
    if (rc != DSH_OK) { err = R[g].c->err; return rc; }
  }
  return DSH_OK;
}

}  // namespace

int dsh_sft_connected_solve(dsh_ctx* c, dsh_comm* cm, const dsh_sft_frame* frame, dsh_sft_result* result) {
  if (!c || !cm || !frame || !result || cm->ctx != c) return dsh_fail(c, DSH_ERR_ARG, "dsh_sft_connected_solve: bad argument");
  if (cm->nranks != 2) return dsh_fail(c, DSH_ERR_ARG, "dsh_sft_connected_solve: the cut has two parts: the communicator must have exactly two ranks");
  std::vector<ScRank> R{ScRank{c}};
  std::string err;
  const int rc = cn_solve(R, cm, cm->rank, frame, result, err);
  return rc == DSH_OK ? rc : dsh_fail(c, rc, "dsh_sft_connected_solve: " + err);
}

int dsh_sft_connected_solve_group(dsh_ctx* c0, dsh_ctx* c1, const dsh_sft_frame* frame, dsh_sft_result* results) {
  if (!c0 || !c1 || c0 == c1 || !frame || !results) return DSH_ERR_ARG;
  std::vector<ScRank> R{ScRank{c0}, ScRank{c1}};
  std::string err;
  const int rc = cn_solve(R, nullptr, 0, frame, results, err);
  return rc == DSH_OK ? rc : dsh_fail(c0, rc, "dsh_sft_connected_solve_group: " + err);
}


}  // extern "C"
