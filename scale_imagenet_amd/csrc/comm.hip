// libttnet.so -- logits all-gather over RCCL (xGMI): the ttnet_comm_* part of include/ttnet.h.
// librccl is resolved at first use so that a process which already carries an RCCL (e.g.
// the one inside PyTorch-ROCm) keeps exactly one copy.

#include <dlfcn.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include "ttnet_common.h"

using namespace ttnet;

extern "C" {

struct ttnet_comm {
  void *nccl = nullptr;
  int rank = 0, world = 1, device = 0;
};

namespace {
struct Id128 {
  char b[128];   // ncclUniqueId, passed by value
};
struct Rccl {
  void *lib = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, Id128, int) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;

int load_rccl() {
  if (g_rccl.lib) return TTNET_OK;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  void *h = nullptr;
  for (const char *nm : names) {
    h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) {
    set_error("cannot load librccl: %s", dlerror());
    return TTNET_E_UNSUPPORTED;
  }
  g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
  g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
  g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
  g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy) {
    set_error("librccl lacks an expected symbol");
    return TTNET_E_UNSUPPORTED;
  }
  g_rccl.lib = h;
  return TTNET_OK;
}

int rccl_check(int r, const char *what) {
  if (r == 0) return TTNET_OK;
  set_error("%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "rccl error");
  return TTNET_E_HIP;
}
}  // namespace

int ttnet_comm_unique_id(void *id128) {
  if (!id128) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  TT_TRY(load_rccl());
  return rccl_check(g_rccl.GetUniqueId(id128), "ncclGetUniqueId");
}

int ttnet_comm_create(const void *id128, int rank, int world, int device, ttnet_comm **out) {
  if (!id128 || !out || world < 1 || rank < 0 || rank >= world) {
    set_error("bad argument to ttnet_comm_create");
    return TTNET_E_INVALID;
  }
  TT_TRY(load_rccl());
  TT_HIP(hipSetDevice(device));
  std::unique_ptr<ttnet_comm> c(new ttnet_comm());
  c->rank = rank; c->world = world; c->device = device;
  Id128 id;
  memcpy(id.b, id128, 128);
  TT_TRY(rccl_check(g_rccl.CommInitRank(&c->nccl, world, id, rank), "ncclCommInitRank"));
  *out = c.release();
  return TTNET_OK;
}

int ttnet_allgather_logits(ttnet_comm *comm, const float *local_dev, int64_t n_local, int64_t n_classes,
                           float *all_dev, void *stream) {
  if (!comm || !local_dev || !all_dev || n_local < 1 || n_classes < 1) {
    set_error("bad argument to ttnet_allgather_logits");
    return TTNET_E_INVALID;
  }
  // ncclFloat32 == 7
  return rccl_check(g_rccl.AllGather(local_dev, all_dev, (size_t)(n_local * n_classes), 7, comm->nccl,
                                     (hipStream_t)stream),
                    "ncclAllGather");
}

void ttnet_comm_destroy(ttnet_comm *comm) {
  if (!comm) return;
  if (comm->nccl && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm->nccl);
  delete comm;
}

}  // extern "C"
