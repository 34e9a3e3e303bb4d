"""The PPO loop with vss_gae (the default on a GPU) and with VSS_GAE=torch (compute_gae and the torch merge of the
terminal values) trains the same bits: equal per-update history, bit-equal agent parameters at the end."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P

pytestmark = pytest.mark.gpu
KEYS = ("v_loss", "pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "mean_return", "episodes",
        "opponent_version")
MIRROR_KEYS = KEYS + ("mean_return_blue", "mean_return_yellow")


def run(argv, keys):
    args = P.parse_args(argv + ["--log", "false", "--kernel-warmup", "false"])
    agent, hist = P.train(args)
    return [p.detach().clone() for p in agent.parameters()], [{k: h[k] for k in keys} for h in hist]


CASES = {
    "sa-form-b": (["--env-id", "sa", "--num-envs", "256", "--num-steps", "8", "--num-updates", "3"], KEYS),
    "sa-form-a": (["--env-id", "sa", "--num-envs", "256", "--num-steps", "8", "--num-updates", "3",
                   "--fused-policy", "false"], KEYS),
    "dma-mirror": (["--env-id", "dma", "--num-envs", "258", "--num-steps", "8", "--num-updates", "3",
                    "--opponent", "mirror"], MIRROR_KEYS),
    "sa-chain-values": (["--env-id", "sa", "--num-envs", "16384", "--num-steps", "4", "--num-updates", "2"], KEYS),
}


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_and_torch_paths_train_the_same_bits(case, monkeypatch):
    argv, keys = CASES[case]
    calls = []
    import vss_amd.returns as R
    real = R.gae
    monkeypatch.setattr(R, "gae", lambda *a, **kw: (calls.append(sorted(k for k in kw if k != "out")), real(*a, **kw))[1])
    monkeypatch.delenv("VSS_GAE", raising=False)
    params, hist = run(argv, keys)
    n_updates = len(hist)
    form = ["next_values"] if case == "sa-form-a" else ["term_values", "v_last"]
    assert calls == [form] * n_updates  # the kernel ran, once per update, in the form the case is for
    monkeypatch.setenv("VSS_GAE", "torch")
    params_t, hist_t = run(argv, keys)
    assert len(calls) == n_updates  # the torch path does not reach the kernel
    assert hist == hist_t
    assert len(params) == len(params_t)
    for a, b in zip(params, params_t):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_an_unknown_vss_gae_value_is_refused(monkeypatch):
    monkeypatch.setenv("VSS_GAE", "numpy")
    with pytest.raises(ValueError, match="VSS_GAE"):
        run(CASES["sa-form-b"][0], KEYS)
