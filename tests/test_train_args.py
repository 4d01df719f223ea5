"""Null-handle rejection of the optimiser, shard and RCCL entry points, without a GPU: every one returns FFVD_EINVAL before any
device work and names ITSELF in ffvd_last_error(NULL) -- most of them build that message from a name handed to a shared check.
The accessors without a status code return 0 / NULL."""
import ctypes as C

import numpy as np
import pytest

from ffvd_amd import _lib

E = _lib.FFVD_EINVAL
H0 = None                                   # the NULL handle


def _calls():
    dp = _lib.dptr
    terms, nll, buf = np.zeros(8), C.c_double(), np.zeros(16)
    noise_arr = np.zeros(4)
    noise = _lib.FfvdParams(logvariance=noise_arr.ctypes.data)
    grads = _lib.FfvdGrads()
    np_, gp, out = C.byref(noise), C.byref(grads), (dp(terms), C.byref(nll))
    adam = (1e-3, 0.9, 0.999, 1e-8, _lib.TRAIN_ALL)
    hmc = (0.01, 0.05, _lib.TRAIN_BITS["logvariance"], 1, np_)
    uid = np.zeros(256, dtype=np.uint8)
    keep = (terms, nll, buf, noise_arr, noise, grads, uid)
    return keep, {
        "ffvd_optimizer_reset": (H0,),
        "ffvd_adam_step": (H0, *adam, *out),
        "ffvd_sghmc_step": (H0, *hmc, *out),
        "ffvd_train_local": (H0, 1),
        "ffvd_train_exchange_get": (H0, dp(buf)),
        "ffvd_train_exchange_set": (H0, dp(buf)),
        "ffvd_adam_apply": (H0, *adam, *out),
        "ffvd_sghmc_apply": (H0, *hmc, *out),
        "ffvd_adam_step_allreduce": (H0, None, 1, *adam, *out),
        "ffvd_sghmc_step_allreduce": (H0, None, 1, *hmc, *out),
        "ffvd_tshard_local": (H0,),
        "ffvd_tshard_get": (H0, dp(buf)),
        "ffvd_tshard_set": (H0, dp(buf)),
        "ffvd_tshard_finish": (H0, *out),
        "ffvd_tshard_finish_grad": (H0, 1, *out),
        "ffvd_tshard_grad_fetch": (H0, dp(terms), gp),
        "ffvd_tshard_adam_apply": (H0, dp(buf), *adam, *out),
        "ffvd_tshard_sghmc_apply": (H0, *hmc, *out),
        "ffvd_elbo_tshard": (H0, None, *out),
        "ffvd_elbo_tshard_grad": (H0, None, 1, *out, gp),
        "ffvd_comm_unique_id": (None,),                      # no handle: a NULL output pointer
        "ffvd_comm_init": (H0, 1, 0, uid.ctypes.data),
        "ffvd_comm_destroy": (H0,),
        "ffvd_allreduce_sum_async": (H0, None, buf.ctypes.data, 16),
        "ffvd_allreduce_sum": (H0, None, dp(buf), 16),
        "ffvd_elbo_allreduce_async": (H0, None, None),
        "ffvd_elbo_allreduce": (H0, None, *out),
    }


@pytest.mark.parametrize("name", sorted(_calls()[1]))
def test_null_handle_is_rejected_under_the_entry_points_own_name(name):
    lib = _lib.load()
    keep, calls = _calls()
    assert lib.ffvd_sync(None) == E and lib.ffvd_last_error(None).startswith(b"ffvd_sync:")      # a known other message first
    assert getattr(lib, name)(*calls[name]) == E
    msg = lib.ffvd_last_error(None).decode()
    assert msg.startswith(name + ":"), msg
    del keep


def test_accessors_without_a_status_code_return_zero_for_a_null_handle():
    lib = _lib.load()
    assert lib.ffvd_tshard_count(None) == 0
    assert lib.ffvd_train_exchange_count(None) == 0
    assert lib.ffvd_train_exchange_ptr(None) is None
    assert lib.ffvd_comm_get(None) is None


def test_every_moved_entry_point_is_covered():
    """The list above against the header: whatever ffvd_abi.h declares under these prefixes is either called with a NULL handle
    or one of the four accessors."""
    moved = [s for s in _lib.exported_symbols()
             if s.startswith(("ffvd_adam_", "ffvd_sghmc_", "ffvd_train_", "ffvd_tshard_", "ffvd_comm_", "ffvd_allreduce_",
                              "ffvd_elbo_allreduce", "ffvd_elbo_tshard", "ffvd_optimizer_"))]
    accessors = {"ffvd_tshard_count", "ffvd_train_exchange_count", "ffvd_train_exchange_ptr", "ffvd_comm_get"}
    assert set(moved) == set(_calls()[1]) | accessors
