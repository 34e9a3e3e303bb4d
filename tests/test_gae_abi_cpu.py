"""CPU-only checks of vss_gae (include/vss.h, csrc/vss_returns.hip): every invalid argument is rejected before any
HIP call, zero sizes return OK without a launch, and the recurrence the header states -- restated in numpy,
float32 operation by operation -- is compute_gae bit for bit, with gamma * lambda formed in double."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from vss_amd import _native as N

FAKE = 4096  # a non-null, aligned address that is never dereferenced: every call below returns before a launch
E_ARG = 1
FORM_A = dict(next_values=FAKE)
FORM_B = dict(term_values=FAKE, v_last=FAKE)


def call(n_steps=8, n_rows=64, rewards=FAKE, values=FAKE, next_values=None, term_values=None, v_last=None, next_dones=FAKE,
         next_timeouts=FAKE, gamma=0.99, gamma_lambda=0.9405, advantages=FAKE, returns=FAKE):
    return N.load().vss_gae(None, n_steps, n_rows, rewards, values, next_values, term_values, v_last, next_dones,
                            next_timeouts, gamma, gamma_lambda, advantages, returns)


def test_vss_gae_is_exported_and_the_abi_version_stays():
    assert "vss_gae" in N.EXPORTED
    assert N.load().vss_abi_version() == 2 == N.ABI_VERSION
    assert N.STATE_CHANNELS == 58 and N.MODE_DMA == 3


@pytest.mark.parametrize("form", [FORM_A, FORM_B])
@pytest.mark.parametrize("name", ["rewards", "values", "next_dones", "next_timeouts", "advantages", "returns"])
def test_null_required_pointer_is_rejected(form, name):
    assert call(**form, **{name: None}) == E_ARG
    assert call(n_steps=0, **form, **{name: None}) == E_ARG  # checked before the zero-size return


def test_exactly_one_form():
    assert call() == E_ARG  # neither
    assert call(**FORM_A, **FORM_B) == E_ARG  # both
    assert call(next_values=FAKE, term_values=FAKE) == E_ARG
    assert call(next_values=FAKE, v_last=FAKE) == E_ARG
    assert call(term_values=FAKE) == E_ARG  # one of the pair without the other
    assert call(v_last=FAKE) == E_ARG


@pytest.mark.parametrize("form,names", [
    (FORM_A, ["rewards", "values", "next_values", "next_dones", "next_timeouts", "advantages", "returns"]),
    (FORM_B, ["rewards", "values", "term_values", "v_last", "next_dones", "next_timeouts", "advantages", "returns"])])
def test_misaligned_pointer_is_rejected(form, names):
    for name in names:
        for off in (1, 2, 3):
            assert call(**{**form, name: FAKE + off}) == E_ARG, (name, off)


@pytest.mark.parametrize("form", [FORM_A, FORM_B])
def test_negative_sizes_and_non_finite_constants_are_rejected(form):
    assert call(n_steps=-1, **form) == E_ARG
    assert call(n_rows=-1, **form) == E_ARG
    assert call(n_steps=-1, n_rows=0, **form) == E_ARG
    assert call(n_steps=0, n_rows=-1, **form) == E_ARG
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(gamma=bad, **form) == E_ARG
        assert call(gamma_lambda=bad, **form) == E_ARG
        assert call(n_rows=0, gamma=bad, **form) == E_ARG


@pytest.mark.parametrize("form", [FORM_A, FORM_B])
def test_zero_sizes_are_ok_without_a_launch(form):
    assert call(n_steps=0, **form) == 0
    assert call(n_rows=0, **form) == 0
    assert call(n_steps=0, n_rows=0, **form) == 0


# ---- the recurrence of include/vss.h in numpy: every operation rounds to float32, in the header's order ----------

def gae_numpy(rewards, values, next_values, next_dones, next_timeouts, gamma, gamma_lambda):
    f = np.float32
    T, E = rewards.shape
    adv, ret = np.empty((T, E), f), np.empty((T, E), f)
    last = np.zeros(E, f)
    g, gl = f(gamma), f(gamma_lambda)
    for t in range(T - 1, -1, -1):
        nnt = np.where((next_dones[t] != 0) & (next_timeouts[t] == 0), f(0), f(1))
        delta = (rewards[t] + (g * next_values[t]) * nnt) - values[t]
        last = delta + (gl * (f(1) - next_dones[t])) * last
        adv[t] = last
        ret[t] = last + values[t]
    return adv, ret


def rollout(T, E, seed):
    rng = np.random.default_rng(seed)
    rewards, values, next_values = (rng.standard_normal((T, E)).astype(np.float32) for _ in range(3))
    u = rng.random((T, E))
    dones = (u < 0.10).astype(np.float32)
    timeouts = ((u < 0.05) | (rng.random((T, E)) < 0.02)).astype(np.float32)  # half of the dones, a few without one
    return rewards, values, next_values, dones, timeouts


def rounded_in_double(gamma, lam):
    return ctypes.c_float(gamma * lam).value


SETTINGS = [(0.99, 0.95), (0.997, 0.9), (1.0, 1.0)]


@pytest.mark.parametrize("gamma,lam", SETTINGS)
@pytest.mark.parametrize("T,E", [(3, 2), (37, 65)])
def test_numpy_restatement_is_compute_gae_bit_for_bit(T, E, gamma, lam):
    data = rollout(T, E, seed=T * 1000 + E)
    adv_t, ret_t = P.compute_gae(*(torch.from_numpy(x) for x in data), gamma, lam)
    r, v, nv, d, o = data
    adv, ret = gae_numpy(r, v, nv, d, o, gamma, rounded_in_double(gamma, lam))
    np.testing.assert_array_equal(adv.view(np.int32), adv_t.numpy().view(np.int32))
    np.testing.assert_array_equal(ret.view(np.int32), ret_t.numpy().view(np.int32))


def test_the_fp32_product_of_gamma_and_lambda_is_another_constant():
    """(0.997, 0.9): float32(gamma) * float32(lambda) differs from the double product rounded once, and the
    recurrence with it is not compute_gae -- the binding must pass the latter."""
    gamma, lam = 0.997, 0.9
    fp32_product = float(np.float32(gamma) * np.float32(lam))
    assert fp32_product != rounded_in_double(gamma, lam)
    data = rollout(37, 65, seed=37065)
    adv_t, _ = P.compute_gae(*(torch.from_numpy(x) for x in data), gamma, lam)
    r, v, nv, d, o = data
    adv, _ = gae_numpy(r, v, nv, d, o, gamma, fp32_product)
    assert not np.array_equal(adv.view(np.int32), adv_t.numpy().view(np.int32))
    for g, l in ((0.99, 0.95), (1.0, 1.0)):  # the other settings do not tell the two apart
        assert float(np.float32(g) * np.float32(l)) == rounded_in_double(g, l)


def test_the_binding_passes_the_double_product():
    from vss_amd.returns import gamma_lambda
    for g, l in SETTINGS:
        assert gamma_lambda(g, l) == rounded_in_double(g, l)


def test_vss_gae_switch_is_read_when_called(monkeypatch):
    from vss_amd.returns import kernel_selected
    monkeypatch.delenv("VSS_GAE", raising=False)
    assert kernel_selected("cuda:0") and not kernel_selected("cpu")
    monkeypatch.setenv("VSS_GAE", "torch")
    assert not kernel_selected("cuda:0") and not kernel_selected("cpu")
    monkeypatch.setenv("VSS_GAE", "numpy")
    with pytest.raises(ValueError, match="VSS_GAE"):
        kernel_selected("cuda:0")
