// Native RCCL collectives of the C ABI (SURVEY 8b `ffvd_elbo_allreduce(h, rccl_comm)`, 8e): the run-time binding of librccl, the
// handle's communicator, all-reduce(sum) on the handle's stream.  The only source that sees <dlfcn.h> and <rccl/rccl.h>.
//
// The only exchange step of the path is an all-reduce(sum) of the 8 partial sums over xGMI.  librccl is bound at run time
// (dlopen): the library that is already mapped in the process wins (a host that also runs PyTorch has torch's bundled
// RCCL mapped, and two RCCL copies in one process must be avoided), then $FFVD_RCCL_LIB, then the system library.  A
// build box or a host without RCCL therefore still loads libffvd_hip.so; the collective entry points then fail loudly.
#include "handle.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <rccl/rccl.h>
#include <string>

using namespace ffvd;

namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
};
void rccl_bind(RcclApi &api);
RcclApi *rccl_api() {
    static RcclApi api;
    static std::once_flag once;             // handles of different threads may ask at the same time
    std::call_once(once, [] { rccl_bind(api); });
    return &api;
}
void rccl_bind(RcclApi &api) {
    const char *env = getenv("FFVD_RCCL_LIB");
    const char *names[] = {"librccl.so.1", "librccl.so"};
    for (const char *n : names)
        if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);           // whatever the process already runs on
    if (!api.lib && env && *env) api.lib = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
    for (const char *n : names)
        if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!api.lib) api.lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!api.lib) {
        const char *why = dlerror();
        api.why = std::string("librccl not found: ") + (why ? why : "?");
        return;
    }
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.GetErrorString) {
        api.why = "librccl lacks an expected symbol";
        api.lib = nullptr;
    }
}
}  // namespace

#define RCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) {                                                                   \
            char buf_[512];                                                                        \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, api->GetErrorString(r_), __FILE__, __LINE__); \
            return set_error(h, FFVD_EDEVICE, buf_);                                               \
        }                                                                                          \
    } while (0)

extern "C" int ffvd_comm_unique_id(void *id_out) {
    ffvd_handle *h = nullptr;
    if (!id_out) return set_error(nullptr, FFVD_EINVAL, "ffvd_comm_unique_id: null argument");
    RcclApi *api = rccl_api();
    if (!api->lib) return set_error(nullptr, FFVD_EDEVICE, "ffvd_comm_unique_id: " + api->why);
    ncclUniqueId id;
    RCCL_TRY(api->GetUniqueId(&id));
    memcpy(id_out, &id, FFVD_COMM_ID_BYTES);
    return FFVD_OK;
}

extern "C" int ffvd_comm_init(ffvd_handle *h, int world, int rank, const void *id) {
    if (!h || !id || world < 1 || rank < 0 || rank >= world)
        return set_error(h, FFVD_EINVAL, "ffvd_comm_init: bad argument");
    if (h->comm) return set_error(h, FFVD_EINVAL, "ffvd_comm_init: the handle already owns a communicator");
    RcclApi *api = rccl_api();
    if (!api->lib) return set_error(h, FFVD_EDEVICE, "ffvd_comm_init: " + api->why);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    ncclUniqueId uid;
    static_assert(sizeof(uid) == FFVD_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(&uid, id, sizeof uid);
    ncclComm_t comm = nullptr;
    RCCL_TRY(api->CommInitRank(&comm, world, uid, rank));
    h->comm = (void *)comm;
    h->comm_world = world;
    h->comm_rank = rank;
    return FFVD_OK;
}

extern "C" int ffvd_comm_destroy(ffvd_handle *h) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_comm_destroy: null handle");
    if (!h->comm) return FFVD_OK;
    RcclApi *api = rccl_api();
    hipSetDevice(h->cfg.device_id);
    hipStreamSynchronize(h->stream);
    ncclComm_t comm = (ncclComm_t)h->comm;
    h->comm = nullptr;
    if (api->lib) RCCL_TRY(api->CommDestroy(comm));
    return FFVD_OK;
}

extern "C" void *ffvd_comm_get(ffvd_handle *h) { return h ? h->comm : nullptr; }

extern "C" int ffvd_allreduce_sum_async(ffvd_handle *h, void *rccl_comm, double *buf_dev, int64_t count) {
    if (!h || !buf_dev || count < 0) return set_error(h, FFVD_EINVAL, "ffvd_allreduce_sum_async: bad argument");
    void *comm = rccl_comm ? rccl_comm : h->comm;
    if (!comm) return set_error(h, FFVD_EINVAL, "ffvd_allreduce_sum_async: no communicator (pass one or call ffvd_comm_init)");
    RcclApi *api = rccl_api();
    if (!api->lib) return set_error(h, FFVD_EDEVICE, "ffvd_allreduce_sum_async: " + api->why);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (count == 0) return FFVD_OK;
    RCCL_TRY(api->AllReduce(buf_dev, buf_dev, (size_t)count, ncclDouble, ncclSum, (ncclComm_t)comm, h->stream));
    return FFVD_OK;
}

extern "C" int ffvd_allreduce_sum(ffvd_handle *h, void *rccl_comm, double *buf_host, int64_t count) {
    if (!h || !buf_host || count < 0) return set_error(h, FFVD_EINVAL, "ffvd_allreduce_sum: bad argument");
    if (count == 0) return FFVD_OK;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (h->stage_count < count) {          // device staging buffer, grown on demand and kept by the handle
        double *d = nullptr;
        HIP_TRY(dev_alloc(h, &d, (size_t)count));
        h->stage = d;
        h->stage_count = count;
    }
    HIP_TRY(hipMemcpyAsync(h->stage, buf_host, (size_t)count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = ffvd_allreduce_sum_async(h, rccl_comm, h->stage, count);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(buf_host, h->stage, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FFVD_OK;
}

extern "C" int ffvd_elbo_allreduce_async(ffvd_handle *h, void *rccl_comm, double *out_terms_dev) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_elbo_allreduce_async: null handle");
    int rc;
    double *dst = out_terms_dev ? out_terms_dev : h->out_terms;
    if ((rc = ffvd_elbo_async(h, dst))) return rc;
    return ffvd_allreduce_sum_async(h, rccl_comm, dst, 8);
}

extern "C" int ffvd_elbo_allreduce(ffvd_handle *h, void *rccl_comm, double out_terms[8], double *out_nll) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_elbo_allreduce: null handle");
    int rc;
    // kernels -> finalize (8 partial sums in HBM) -> ncclAllReduce on the same stream -> one copy back: the only host
    // synchronisation of the step is the final one
    if ((rc = ffvd_elbo_allreduce_async(h, rccl_comm, nullptr))) return rc;
    h->info_pending = false;
    HIP_TRY(hipMemcpyAsync(h->h_res, h->resblk, h->res_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = check_info(h))) return rc;              // this rank's factorisations
    // a failed factorisation on ANOTHER rank poisons the sums with NaN
    if ((rc = check_finite(h, h->h_out, 8, "ffvd_elbo_allreduce",
                           "partial sums after the all-reduce (a factorisation failed or was abandoned on another rank)")))
        return rc;
    report_sums(h->h_out, out_terms, out_nll);
    return FFVD_OK;
}
