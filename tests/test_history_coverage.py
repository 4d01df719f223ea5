"""CPU: the two lists of the history tests cannot rot.  Every buffer a handle allocates (dev_alloc in the handle's sources) must be
named by a configuration of tests/test_gpu_history.py, and every `ffvd_op_*` entry point of include/ffvd_abi.h must be called by
tests/cache_poison_script.py or be exempt for a stated reason: a new buffer or operator fails here until someone says which case
covers it."""
import os
import re

import cache_poison_script as script
import test_gpu_history as history
from conftest import ROOT

CSRC = os.path.join(ROOT, "ffvd_amd", "csrc")
HANDLE_SOURCES = ("handle.h", "abi.hip", "backward.hip", "train.hip", "comm.hip")

# entry points the poison script does not call, and why
EXEMPT = {
    "ffvd_op_release_cache": "frees the cache itself, takes no scratch (the script calls it last, after the outputs are formed)",
    "ffvd_op_rollout_fallbacks": "reads a host counter of the resident rollout loop, no device work",
}


def allocated_buffers():
    """NAME of every dev_alloc(h, &h->NAME / &g.NAME / &NAME ...) in the sources that see inside the handle (array members without
    their index)"""
    names = {}
    for src in HANDLE_SOURCES:
        with open(os.path.join(CSRC, src)) as f:
            text = f.read()
        for m in re.finditer(r"dev_alloc\(h,\s*&(?:h->|g\.)?([A-Za-z_][A-Za-z_0-9]*)", text):
            names.setdefault(m.group(1), src)
    return names


def declared_operators():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        return sorted(set(re.findall(r"\b(ffvd_op_[a-z_0-9]+)\s*\(", f.read())))


def test_every_handle_buffer_is_covered_by_a_history_configuration():
    names = allocated_buffers()
    assert len(names) > 80 and "Linv" in names and "pack" in names and "hmc" in names and "d" in names     # the parser still finds them
    assert set(history.COVERS) == set(history.CONFIGS)
    covered = set().union(*history.COVERS.values())
    missing = {n: src for n, src in names.items() if n not in covered}
    assert not missing, f"no configuration of tests/test_gpu_history.py covers {missing}: add the buffer to COVERS (and a configuration that reaches it)"
    unknown = covered - set(names)
    assert not unknown, f"COVERS names buffers no source allocates: {sorted(unknown)}"


def test_every_operator_entry_point_runs_poisoned_or_is_exempt():
    ops = declared_operators()
    assert len(ops) > 50 and "ffvd_op_forecast_particle_grouped" in ops
    called = set(script.called_symbols())
    assert not (called & set(EXEMPT)), "an exempt entry point is called after all: drop the exemption"
    missing = [s for s in ops if s not in called and s not in EXEMPT]
    assert not missing, f"tests/cache_poison_script.py calls none of {missing}: add a call, or an exemption with its reason"
    stale = sorted((called | set(EXEMPT)) - set(ops))
    assert not stale, f"not in include/ffvd_abi.h: {stale}"


def test_the_coincident_inducing_points_failure_runs_wherever_k_uu_allows_it():
    """`dupz` of a configuration is no opinion: it is set exactly where K_uu(Z) of the row's SE kernels is positive definite without
    jitter by a margin fp64 keeps (lambda_min / lambda_max > DUPZ_MIN_EIG_RATIO, eigenvalues by numpy on the CPU), so that handles
    created with jitter = 0.0 can evaluate p1.  A row that leaves the failure out has to be one that cannot."""
    for key, cfg in history.CONFIGS.items():
        ratio = history.k_uu_eig_ratio(key)
        allowed = ratio is not None and ratio > history.DUPZ_MIN_EIG_RATIO
        assert bool(cfg.get("dupz")) == allowed, (key, ratio)
        if allowed:
            assert ratio > 1.2 * history.DUPZ_MIN_EIG_RATIO, (key, ratio)       # no row sits on the threshold itself
