// What the two halves of the C ABI share: abi.hip with backward.hip, train.hip and comm.hip (handles, the ELBO iteration and its
// backward pass, training, shards, RCCL) and ops.hip, ops_loops.hip, ops_grouped.hip (the stateless ffvd_op_* operators).  Error reporting and the guard around a
// forced Cholesky variant; nothing else crosses between them.
#pragma once
#include "../../include/ffvd_abi.h"
#include "kernels.h"

#include <cstddef>
#include <cstdio>
#include <string>

namespace ffvd {

// the calling thread's error / warning string (what ffvd_last_error(NULL) returns); defined once, in abi.hip
std::string &last_error();
// records msg (in the handle as well when there is one) and returns code
int set_error(ffvd_handle *h, int code, const std::string &msg);      // abi.hip; the handle is defined in handle.h, which the operator sources do not include
inline int set_error(std::nullptr_t, int code, const std::string &msg) {
    last_error() = msg;
    return code;
}

// return from the calling function with FFVD_ENOMEM / FFVD_EDEVICE when a HIP call fails; h_: the handle whose error string is set, or nullptr
#define HIP_TRY_ON(h_, expr, text)                                                            \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            char buf_[512];                                                                   \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", text, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                     \
            return ffvd::set_error(h_, (e_ == hipErrorOutOfMemory) ? FFVD_ENOMEM : FFVD_EDEVICE, buf_); \
        }                                                                                     \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_ON(h, expr, #expr)            // where a handle `h` is in scope
#define OP_TRY(expr) HIP_TRY_ON(nullptr, expr, #expr)       // the operators: no handle

// The Cholesky variant override is thread-local state: it is reset on EVERY exit path of the scope that set it (an error
// return between set and reset left the launch-per-column variant selected for every later factorisation of the thread).
struct CholOverrideGuard {
    bool armed = false;
    void force_left() { potrf_override_variant(CHOL_FORCE_LEFT); armed = true; }
    ~CholOverrideGuard() { if (armed) potrf_override_variant(CHOL_FORCE_NONE); }
};

}  // namespace ffvd
