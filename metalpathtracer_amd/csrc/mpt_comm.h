// mpt_comm.h — multi-GPU: the RCCL reduce of the HDR sum behind mpt_comm_* (include/mpt.h).  librccl is loaded on first use (dlopen), so
// a single-GPU program never needs it.  Host code only: mpt_hip.hip includes it once, behind every entry point of a context.
#pragma once

#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static const char* rccl_load() {  // nullptr = ok, else what failed
    if (g_rccl.lib) return nullptr;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return "librccl.so not found";
    RcclApi a;
    a.lib = h;
#define MPT_SYM(field, name)                                 \
    *(void**)(&a.field) = dlsym(h, name);                    \
    if (!a.field) {                                          \
        dlclose(h);                                          \
        return "librccl.so lacks " name;                     \
    }
    MPT_SYM(GetUniqueId, "ncclGetUniqueId")
    MPT_SYM(CommInitAll, "ncclCommInitAll")
    MPT_SYM(CommInitRank, "ncclCommInitRank")
    MPT_SYM(CommDestroy, "ncclCommDestroy")
    MPT_SYM(CommAbort, "ncclCommAbort")
    MPT_SYM(Reduce, "ncclReduce")
    MPT_SYM(GroupStart, "ncclGroupStart")
    MPT_SYM(GroupEnd, "ncclGroupEnd")
    MPT_SYM(GetErrorString, "ncclGetErrorString")
#undef MPT_SYM
    g_rccl = a;
    return nullptr;
}
}  // namespace
static_assert(sizeof(ncclUniqueId) == MPT_COMM_ID_BYTES, "MPT_COMM_ID_BYTES must match ncclUniqueId");

struct mpt_comm {
    std::vector<mpt_ctx*> ctxs;      // local contexts (all N in one process, or this rank's one)
    std::vector<ncclComm_t> comms;   // one per local context; empty when nranks == 1
    int nranks = 1, first_rank = 0;  // global size; global rank of ctxs[0]
    bool aborted = false;            // a local failure aborted the communicators: nothing more can be reduced
    std::string err;
};

extern "C" const char* mpt_comm_last_error(const mpt_comm* c) { return c ? c->err.c_str() : "null communicator"; }

extern "C" int mpt_comm_unique_id(void* id_out) {
    if (!id_out) return MPT_ERR_INVALID_ARG;
    if (rccl_load()) return MPT_ERR_HIP;
    ncclUniqueId id;
    if (g_rccl.GetUniqueId(&id) != ncclSuccess) return MPT_ERR_HIP;
    memcpy(id_out, &id, sizeof id);
    return MPT_OK;
}

extern "C" int mpt_comm_create_all(mpt_ctx* const* ctxs, int n, mpt_comm** out) {
    if (!out) return MPT_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ctxs || n < 1) return MPT_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]) return MPT_ERR_INVALID_ARG;
    try {
        std::unique_ptr<mpt_comm> c(new mpt_comm());
        c->ctxs.assign(ctxs, ctxs + n);
        c->nranks = n;
        if (n > 1) {
            if (const char* why = rccl_load()) return fail(ctxs[0], MPT_ERR_HIP, why);
            std::vector<int> devs(n);
            for (int i = 0; i < n; ++i) devs[i] = ctxs[i]->device;
            c->comms.resize(n);
            ncclResult_t r = g_rccl.CommInitAll(c->comms.data(), n, devs.data());
            if (r != ncclSuccess) return fail(ctxs[0], MPT_ERR_HIP, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r));
        }
        *out = c.release();
        return MPT_OK;
    } catch (...) {
        return MPT_ERR_HIP;
    }
}

extern "C" int mpt_comm_create_rank(mpt_ctx* ctx, int rank, int nranks, const void* id, mpt_comm** out) {
    if (!out) return MPT_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ctx || nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !id)) return MPT_ERR_INVALID_ARG;
    try {
        std::unique_ptr<mpt_comm> c(new mpt_comm());
        c->ctxs.push_back(ctx);
        c->nranks = nranks;
        c->first_rank = rank;
        if (nranks > 1) {
            if (const char* why = rccl_load()) return fail(ctx, MPT_ERR_HIP, why);
            if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, MPT_ERR_HIP, "hipSetDevice failed");
            ncclUniqueId uid;
            memcpy(&uid, id, sizeof uid);
            c->comms.resize(1);
            ncclResult_t r = g_rccl.CommInitRank(&c->comms[0], nranks, uid, rank);
            if (r != ncclSuccess) return fail(ctx, MPT_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
        }
        *out = c.release();
        return MPT_OK;
    } catch (...) {
        return MPT_ERR_HIP;
    }
}

// A rank that cannot enter the collective must not leave its peers waiting in it: the local communicators are aborted
// (ncclCommAbort), which makes the peers' ncclReduce fail instead of hanging on their GPUs.  The job is over then — the
// communicator cannot be used again (mpt_reduce_sum returns MPT_ERR_NOT_READY on it), the caller tears down and restarts.
static void comm_abort(mpt_comm* c) {
    for (ncclComm_t& k : c->comms) {
        if (k && g_rccl.CommAbort) g_rccl.CommAbort(k);
        k = nullptr;
    }
    c->aborted = true;
}

extern "C" int mpt_reduce_sum(mpt_comm* c, int root) {
    if (!c || root < 0 || root >= c->nranks) return MPT_ERR_INVALID_ARG;
    if (c->aborted) {
        c->err = "communicator was aborted by an earlier failure";
        return MPT_ERR_NOT_READY;
    }
    // every local context: collect the renders in flight (their resolves have then updated the HDR sum)
    int local_rc = MPT_OK;
    for (mpt_ctx* ctx : c->ctxs) {
        int rc = drain_submit(ctx);
        if (!rc) rc = wait_impl(ctx);
        if (rc) {
            c->err = ctx->err;
            local_rc = rc;
            break;
        }
        if (!ctx->d_sum || ctx->W != c->ctxs[0]->W || ctx->H != c->ctxs[0]->H) {
            c->err = "contexts of a communicator must be sized alike (mpt_resize)";
            local_rc = MPT_ERR_NOT_READY;
            break;
        }
    }
    if (local_rc) {
        if (c->nranks > 1) comm_abort(c);
        return local_rc;
    }
    if (c->nranks == 1) return MPT_OK;  // one GPU holds the whole image already
    const size_t count = (size_t)c->ctxs[0]->W * c->ctxs[0]->H * 4;
    ncclResult_t r = g_rccl.GroupStart();
    if (r == ncclSuccess) {   // (GroupEnd always follows a successful GroupStart)
        for (size_t i = 0; i < c->ctxs.size() && r == ncclSuccess; ++i) {
            mpt_ctx* ctx = c->ctxs[i];
            if (hipSetDevice(ctx->device) != hipSuccess) r = ncclUnhandledCudaError;
            else r = g_rccl.Reduce(ctx->d_sum, ctx->d_sum, count, ncclFloat32, ncclSum, root, c->comms[i], ctx->stream);
        }
        ncclResult_t e = g_rccl.GroupEnd();
        if (r == ncclSuccess) r = e;
    }
    if (r != ncclSuccess) {
        c->err = std::string("ncclReduce: ") + g_rccl.GetErrorString(r);
        comm_abort(c);
        return MPT_ERR_HIP;
    }
    for (mpt_ctx* ctx : c->ctxs) {
        if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            c->err = "stream synchronisation after ncclReduce failed";
            comm_abort(c);
            return MPT_ERR_HIP;
        }
    }
    return MPT_OK;
}

extern "C" int mpt_comm_destroy(mpt_comm* c) {
    if (!c) return MPT_ERR_INVALID_ARG;
    for (ncclComm_t k : c->comms)
        if (k && g_rccl.CommDestroy) g_rccl.CommDestroy(k);
    delete c;
    return MPT_OK;
}
