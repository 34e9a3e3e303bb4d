"""The training state file of `--checkpoint-every` / `--resume` (ppo_continuous_action_isaacgym.py).

One `torch.save` dict of CPU tensors and plain Python values (it loads with `weights_only=True`), written
atomically: a temporary file in the same directory, flush + fsync, then `os.replace`, so a kill during the
write leaves the previous state file as it was.  Each owner of state -- VSS, the fused and mirror wrappers,
RecordEpisodeStatisticsTorch, FusedPolicy, SnapshotOpponent, OpponentPool, FlatAdam -- has a `state_dict()` /
`load_state_dict()` pair built on `to_cpu` and `copy_into` below; the train loop puts them together.

    save_state(path, state)                      # adds FORMAT_VERSION and the library's source hash
    state = load_state(path)                     # refuses another FORMAT_VERSION
    check_compatible(state["args"], args)        # ValueError on a structural difference
"""
from __future__ import annotations

import os
import random
import time

import numpy as np
import torch

FORMAT_VERSION = 1

# what the saved buffers' shapes, the Philox keys and the set of state owners are built from: these must
# equal the saved ones (the seed too: the env's Philox key and the policies' seeds are rebuilt from it)
STRUCTURAL = ("env_id", "num_envs", "num_steps", "seed", "opponent", "opponent_pool_slots", "opponent_pool_size",
              "fused_policy", "amp", "cuda")
# the perception channel's flags (vss_amd/perceive.py): structural as well -- the ring's depth and the set of state
# owners follow them -- and absent from a state file written before they existed, where they count as zero
PERCEPTION_STRUCTURAL = ("obs_delay", "obs_noise_pos", "obs_noise_vel", "obs_noise_ang", "obs_noise_angvel")
# the actuation channel's flags (vss_amd/actuate.py): structural in the same way, zero where a state file lacks them
ACTUATION_STRUCTURAL = ("act_gain", "act_noise", "act_levels", "act_deadband", "act_loss")
# the estimation channel's flag (vss_amd/estimate.py): structural in the same way, 0 where a state file lacks it
ESTIMATION_STRUCTURAL = ("obs_predict",)
# the tracking channel's flags (vss_amd/track.py): structural in the same way; a state file that lacks one has its default
TRACKING_STRUCTURAL = ("obs_filter_team", "obs_filter_opp", "obs_filter_ball", "obs_filter_gate_pos", "obs_filter_gate_vel")
TRACKING_DEFAULTS = dict(obs_filter_team=0.0, obs_filter_opp=0.0, obs_filter_ball=0.0, obs_filter_gate_pos=0.03,
                         obs_filter_gate_vel=0.5)
# the set plays' flags (vss_amd/setplay.py): structural in the same way -- the stager is a state owner and its table
# decides every staged episode; a state file that lacks one has its default
SETPLAY_STRUCTURAL = ("setplay_share", "setplay_mix", "setplay_file")
SETPLAY_DEFAULTS = dict(setplay_share=0.0, setplay_mix=None, setplay_file=None)
# the referee's flags (vss_amd/referee.py): structural in the same way -- the referee is a state owner and its
# thresholds decide every stoppage; a state file that lacks one has its default
REFEREE_STRUCTURAL = ("ref_stall_steps", "ref_stall_speed", "ref_area_steps", "ref_area_depth", "ref_area_width", "ref_max_stops")
REFEREE_DEFAULTS = dict(ref_stall_steps=0, ref_stall_speed=0.05, ref_area_steps=0, ref_area_depth=0.15, ref_area_width=0.70,
                        ref_max_stops=0)
# set by train() itself or about the checkpoint, not hyper-parameters: never reported as changed
_NOT_COMPARED = ("resume", "kernel_warmup_s", "graph_prepare_s")


def add_actuation_arguments(p):
    """The command line's actuation flags, all 0 by default: the keys of ACTUATION_STRUCTURAL (envs/wrappers.py Actuated).
    Returns the parser."""
    p.add_argument("--act-gain", type=float, default=0.0, help="actuation: std of the per-episode wheel gains (0..0.3)")
    p.add_argument("--act-noise", type=float, default=0.0, help="actuation: std of the per-step noise on every applied command")
    p.add_argument("--act-levels", type=int, default=0, help="actuation: commands are multiples of 1 / levels (127: 8 bits); 0: exact")
    p.add_argument("--act-deadband", type=float, default=0.0, help="actuation: a received command below this does not move the wheel")
    p.add_argument("--act-loss", type=float, default=0.0, help="actuation: a team's packet is lost with this probability per step")
    return p


def add_estimation_arguments(p):
    """The command line's estimation flag, 0 by default: the key of ESTIMATION_STRUCTURAL (envs/wrappers.py Estimated).
    Returns the parser."""
    p.add_argument("--obs-predict", type=int, default=0, choices=(0, 1),
                   help="1: roll the delayed rows of --obs-delay forward to the present with the drive model (Estimated)")
    return p


def add_tracking_arguments(p):
    """The command line's tracking flags: the keys of TRACKING_STRUCTURAL with TRACKING_DEFAULTS (envs/wrappers.py
    Tracked).  Returns the parser."""
    d = TRACKING_DEFAULTS
    p.add_argument("--obs-filter-team", type=float, default=d["obs_filter_team"],
                   help="tracking: the filter's gain on the own robots, in [0, 1]; 0: not filtered (Tracked)")
    p.add_argument("--obs-filter-opp", type=float, default=d["obs_filter_opp"], help="tracking: the gain on the opponents")
    p.add_argument("--obs-filter-ball", type=float, default=d["obs_filter_ball"], help="tracking: the gain on the ball")
    p.add_argument("--obs-filter-gate-pos", type=float, default=d["obs_filter_gate_pos"],
                   help="tracking: a body further than this (m, x or y) from its prediction is re-initialised; 0: off")
    p.add_argument("--obs-filter-gate-vel", type=float, default=d["obs_filter_gate_vel"],
                   help="tracking: the same for the velocity (m/s); 0: off")
    return p


def add_setplay_arguments(p):
    """The command line's set-play flags: the keys of SETPLAY_STRUCTURAL (envs/wrappers.py set_setplays) and the
    arena's --eval-setplays.  Returns the parser."""
    p.add_argument("--setplay-share", type=float, default=0.0,
                   help="set plays: the share of episodes that start from a named placement (0: none, the default)")
    p.add_argument("--setplay-mix", type=str, default=None,
                   help="set plays: name:weight,... e.g. kickoff:1,free_ball:2,penalty_for:1 (default: every built-in at 1)")
    p.add_argument("--setplay-file", type=str, default=None, help="set plays: a JSON file of custom plays (settings only)")
    p.add_argument("--eval-setplays", type=str, default="",
                   help="arena: also score the agent from each of these set plays, e.g. penalty_for,penalty_against")
    return p


def add_referee_arguments(p):
    """The command line's referee flags: the keys of REFEREE_STRUCTURAL with REFEREE_DEFAULTS (envs/wrappers.py
    set_referee).  Returns the parser."""
    d = REFEREE_DEFAULTS
    p.add_argument("--ref-stall-steps", type=int, default=d["ref_stall_steps"],
                   help="referee: a free ball after the ball has been slower than --ref-stall-speed for this many steps (0: off)")
    p.add_argument("--ref-stall-speed", type=float, default=d["ref_stall_speed"], help="referee: the stuck ball's speed (m/s)")
    p.add_argument("--ref-area-steps", type=int, default=d["ref_area_steps"],
                   help="referee: a penalty (goal kick) after two defenders (attackers) have stood in a goal area with the "
                        "ball for this many steps (0: off)")
    p.add_argument("--ref-area-depth", type=float, default=d["ref_area_depth"], help="referee: the goal area's depth (m)")
    p.add_argument("--ref-area-width", type=float, default=d["ref_area_width"], help="referee: the goal area's width (m)")
    p.add_argument("--ref-max-stops", type=int, default=d["ref_max_stops"], help="referee: calls per episode (0: no cap)")
    return p


def add_channel_arguments(p):
    """The actuation, the estimation, the tracking, the set-play and the referee flags.  Returns the parser."""
    return add_referee_arguments(add_setplay_arguments(add_tracking_arguments(add_estimation_arguments(
        add_actuation_arguments(p)))))


def check_tracking(args):
    """Refuse tracking gains outside [0, 1], negative or non-finite gates, and a gain without vision noise: the filter
    averages noise across frames, and with every --obs-noise-* at 0 there is nothing to filter.  Returns args."""
    get = lambda k: float(TRACKING_DEFAULTS[k] if getattr(args, k, None) is None else getattr(args, k))  # noqa: E731
    gains = [get(k) for k in TRACKING_STRUCTURAL[:3]]
    for k, g in zip(TRACKING_STRUCTURAL[:3], gains):
        if not 0.0 <= g <= 1.0:
            raise ValueError(f"--{k.replace('_', '-')} must be in [0, 1], got {g}")
    for k in TRACKING_STRUCTURAL[3:]:
        if not 0.0 <= get(k) < float("inf"):
            raise ValueError(f"--{k.replace('_', '-')} must be finite and >= 0, got {get(k)}")
    if any(gains) and not any(float(getattr(args, f"obs_noise_{k}", 0.0) or 0.0) for k in ("pos", "vel", "ang", "angvel")):
        raise ValueError("--obs-filter-* needs vision noise (--obs-noise-pos / -vel / -ang / -angvel): the tracker "
                         "filters noise across frames, and without noise there is nothing to filter")
    return args


def check_estimation(args):
    """Refuse --obs-predict 1 without latency.  Returns args."""
    predict = int(getattr(args, "obs_predict", 0) or 0)
    if predict not in (0, 1):
        raise ValueError(f"--obs-predict must be 0 or 1, got {predict}")
    if predict and int(getattr(args, "obs_delay", 0) or 0) < 1:
        raise ValueError("--obs-predict 1 needs --obs-delay of at least 1: the predictor rolls a delayed observation "
                         "forward by its age, and with --obs-delay 0 every row is current, so there is nothing to predict")
    return args


def opponent_mode(value) -> str:
    """--opponent as a structural value: ou / self / pool / mirror / scripted, or 'checkpoint' for any path."""
    value = "ou" if value is None else str(value)
    return value if value in ("ou", "self", "pool", "mirror", "scripted") else "checkpoint"


def plain_args(args) -> dict:
    """vars(args) restricted to what a weights_only load takes back: None, bool, int, float and str."""
    d = args if isinstance(args, dict) else vars(args)
    return {k: v for k, v in d.items() if v is None or isinstance(v, (bool, int, float, str))}


def check_compatible(saved_args, args, log=print) -> list:
    """Compare a state file's args with this command line's.  A structural argument that differs raises a
    ValueError naming the key and both values; every other argument is taken from `args`, and each one that
    differs from the saved value is reported once through `log` (None: silent).  Returns the changed keys."""
    saved, new = plain_args(saved_args), plain_args(args)
    for k in (STRUCTURAL + PERCEPTION_STRUCTURAL + ACTUATION_STRUCTURAL + ESTIMATION_STRUCTURAL + TRACKING_STRUCTURAL
              + SETPLAY_STRUCTURAL + REFEREE_STRUCTURAL):
        a, b = saved.get(k), new.get(k)
        if k == "opponent":
            a, b = opponent_mode(a), opponent_mode(b)
        if k in PERCEPTION_STRUCTURAL + ACTUATION_STRUCTURAL + ESTIMATION_STRUCTURAL:
            a, b = a or 0, b or 0
        if k in TRACKING_STRUCTURAL:
            a, b = (TRACKING_DEFAULTS[k] if v is None else v for v in (a, b))
        if k == "setplay_share":
            a, b = float(a or 0.0), float(b or 0.0)
        if k in SETPLAY_STRUCTURAL[1:]:
            a, b = a or None, b or None
        if k in REFEREE_STRUCTURAL:
            a, b = (type(REFEREE_DEFAULTS[k])(REFEREE_DEFAULTS[k] if v is None else v) for v in (a, b))
        if a != b:
            raise ValueError(f"--resume: {k} is structural and differs: the state file has {a!r}, this command line {b!r}")
    changed = []
    for k in sorted(set(saved) | set(new)):
        if k in _NOT_COMPARED:  # (a structural key that differs here: another path of a checkpoint opponent)
            continue
        a, b = saved.get(k), new.get(k)
        if a != b and not (isinstance(a, float) and isinstance(b, float) and a != a and b != b):
            changed.append(k)
            if log is not None:
                log(f"--resume: {k} changed from {a!r} (saved) to {b!r}; the new value is used")
    return changed


def source_hash() -> str:
    from . import _native
    return _native.source_hash()


def _write(obj, f) -> None:
    torch.save(obj, f)


def atomic_save(path: str, obj) -> int:
    """torch.save(obj) to `path` through a temporary file in the same directory: flush + fsync, then
    os.replace.  A failure or a kill on the way leaves `path` as it was.  Returns the file's size in bytes."""
    path = os.path.abspath(path)
    folder = os.path.dirname(path)
    os.makedirs(folder, exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            _write(obj, f)
            f.flush()
            os.fsync(f.fileno())
        size = os.path.getsize(tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    fd = os.open(folder, os.O_RDONLY)  # the rename itself
    try:
        os.fsync(fd)
    finally:
        os.close(fd)
    return size


def save_state(path: str, state: dict) -> int:
    """Write `state` (+ format_version, source_hash) to `path` atomically; returns the file's size in bytes."""
    return atomic_save(path, dict(state, format_version=FORMAT_VERSION,
                                  source_hash=state.get("source_hash") or source_hash()))


def load_state(path: str) -> dict:
    """The state dict of `path` on the CPU; a file of another FORMAT_VERSION (or none) is refused."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    version = state.get("format_version") if isinstance(state, dict) else None
    if version != FORMAT_VERSION:
        raise ValueError(f"{path}: state format version {version!r}, this build reads version {FORMAT_VERSION}")
    return state


# ---- building blocks of the owners' state_dict() / load_state_dict() -----------------------------------------
def to_cpu(tree):
    """A copy of a tree of dicts / lists / tuples with every tensor detached onto the CPU."""
    if isinstance(tree, torch.Tensor):
        return tree.detach().to("cpu", copy=True)
    if isinstance(tree, dict):
        return {k: to_cpu(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [to_cpu(v) for v in tree]
    return tree


def copy_into(dst: torch.Tensor, src, name: str) -> None:
    """dst.copy_(src) after checking shape and dtype: the existing tensor, and every view of it, stays."""
    if not isinstance(src, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(src).__name__}")
    if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        raise ValueError(f"{name}: saved {tuple(src.shape)} {src.dtype} does not fit {tuple(dst.shape)} {dst.dtype}")
    with torch.no_grad():
        dst.copy_(src)


def entry(state: dict, key: str, owner: str):
    if not isinstance(state, dict) or key not in state:
        raise ValueError(f"{owner}: the saved state has no entry {key!r}")
    return state[key]


def copy_entries(owner: str, tensors: dict, state: dict) -> None:
    """copy_into for every named tensor of an owner (None: the owner does not have it, nothing is read)."""
    for k, dst in tensors.items():
        if dst is not None:
            copy_into(dst, entry(state, k, owner), f"{owner}.{k}")


def python_rng_state(state=None) -> list:
    """random.getstate() (or the given one) as nested lists."""
    version, internal, gauss = random.getstate() if state is None else state
    return [version, list(internal), gauss]


def python_rng_tuple(saved) -> tuple:
    version, internal, gauss = saved
    return (int(version), tuple(int(v) for v in internal), gauss)


def numpy_rng_state() -> list:
    name, keys, pos, has_gauss, cached = np.random.get_state()
    return [str(name), torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(cached)]


def numpy_rng_tuple(saved) -> tuple:
    name, keys, pos, has_gauss, cached = saved
    return (str(name), np.asarray(keys, dtype=np.int64).astype(np.uint32), int(pos), int(has_gauss), float(cached))


def rng_state(gen: torch.Generator, device) -> dict:
    """Every generator the loop or the code under it may draw from: reading a state consumes nothing."""
    device = torch.device(device)
    return {"gen": gen.get_state().clone(), "python": python_rng_state(), "numpy": numpy_rng_state(),
            "torch_cpu": torch.get_rng_state().clone(),
            "torch_device": torch.cuda.get_rng_state(device).clone() if device.type == "cuda" else None}


def load_rng_state(saved: dict, gen: torch.Generator, device) -> None:
    device = torch.device(device)
    gen.set_state(entry(saved, "gen", "rng"))
    random.setstate(python_rng_tuple(entry(saved, "python", "rng")))
    np.random.set_state(numpy_rng_tuple(entry(saved, "numpy", "rng")))
    torch.set_rng_state(entry(saved, "torch_cpu", "rng"))
    if device.type == "cuda" and saved.get("torch_device") is not None:
        torch.cuda.set_rng_state(saved["torch_device"], device)


# ---- the train loop's side (ppo_continuous_action_isaacgym.py train) ---------------------------------------------
def checkpoint_paths(args, run_name: str, update: int | None = None):
    """(the state file, the agent file of `update`) of --checkpoint-every, both in the run's directory."""
    folder = f"{args.save_path}/{run_name}"
    return f"{folder}/{run_name}-state.pt", None if update is None else f"{folder}/{run_name}-agent-u{update:06d}.pt"


def begin(args):
    """Before any GPU work or process group: refuse what is not built, and with --resume read the state file
    and compare its command line with this one.  Returns the saved state, or None without --resume."""
    every, path = int(getattr(args, "checkpoint_every", 0) or 0), getattr(args, "resume", None)
    if every < 0:
        raise ValueError(f"--checkpoint-every must be >= 0, got {every}")
    if (every or path) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--checkpoint-every / --resume with WORLD_SIZE > 1: per-rank state files are not built "
                         "(the env state, the Philox counters and a league's tallies are per rank); run them on one rank")
    if not path:
        return None
    saved = load_state(path)
    check_compatible(entry(saved, "args", "state"), args)
    if saved.get("source_hash") != source_hash():
        print(f"--resume: {path} was written by a library built from other sources ({saved.get('source_hash')}, here "
              f"{source_hash()}): a bit-equal continuation is no longer promised", flush=True)
    if getattr(args, "log", False):
        print(f"--resume: {path}, update {saved['update']}, step {saved['global_step']}", flush=True)
    return saved


def owners(optimizer, env, wrapper, episode_stats, fused=None, opponent=None) -> dict:
    """What carries state from one update to the next, each with a state_dict() / load_state_dict() pair."""
    out = {"optimizer": optimizer, "env": env, "wrapper": wrapper, "episode_stats": episode_stats}
    if fused is not None:
        out["fused_policy"] = fused
    if opponent is not None:
        out["opponent"] = opponent
    return out


def training_state(args, agent, owners: dict, gen, device, update: int, global_step: int, wall_s: float,
                   history: list) -> dict:
    """Everything the next update depends on, as CPU tensors and plain values: the agent's
    parameters, each owner's state_dict(), every generator's state and the loop's scalars.  Reading it draws no
    random number and rebinds no buffer."""
    return {"args": plain_args(args), "agent": to_cpu(dict(agent.state_dict())),
            "owners": {k: o.state_dict() for k, o in owners.items()}, "rng": rng_state(gen, device),
            "update": int(update), "global_step": int(global_step), "wall_s": float(wall_s),
            "history": [dict(r) for r in history]}


def load_training_state(state: dict, agent, owners: dict, gen, device) -> None:
    """Put a training_state() back: every tensor is copied into the one that exists (the agent's parameters stay
    views of the flat buffer), the generators last."""
    copy_entries("agent", dict(agent.state_dict()), entry(state, "agent", "state"))
    saved = entry(state, "owners", "state")
    if sorted(saved) != sorted(owners):
        raise ValueError(f"--resume: the state file holds {sorted(saved)}, this run has {sorted(owners)}")
    for k, o in owners.items():
        o.load_state_dict(saved[k])
    load_rng_state(entry(state, "rng", "state"), gen, device)


def resume(saved, agent, owners: dict, gen, device, start_time: float):
    """(first update, global_step, history, start_time) of the loop: 1, 0, [] and the given clock without a
    saved state; else the state is loaded and the loop goes on after the saved update, on the saved clock
    (wall_s and sps include the time before the interruption)."""
    if saved is None:
        return 1, 0, [], start_time
    load_training_state(saved, agent, owners, gen, device)
    return (int(saved["update"]) + 1, int(saved["global_step"]), [dict(r) for r in saved["history"]],
            time.time() - float(saved["wall_s"]))


def checkpoint(args, rank: int, run_name: str, rec: dict, agent, owners: dict, gen, device, history: list,
               start_time: float) -> int:
    """The end of an update's bookkeeping: on every --checkpoint-every-th update rank 0 writes the state file and
    the agent file.  Sets rec["checkpoint_s"] (0.0 when nothing was written) and, after a write, rec["wall_s"] and
    rec["sps"], which include it; returns rec["sps"].  The state file's own copy of this record keeps
    checkpoint_s 0.0 and the clock from before the write."""
    rec["checkpoint_s"] = 0.0
    every, update = int(getattr(args, "checkpoint_every", 0) or 0), rec["update"]
    if every and update % every == 0 and rank == 0:
        t0 = time.time()
        state_path, agent_path = checkpoint_paths(args, run_name, update)
        save_state(state_path, training_state(args, agent, owners, gen, device, update, rec["global_step"], rec["wall_s"],
                                              history))
        atomic_save(agent_path, agent.state_dict())  # the reference's format: play.py, --opponent PATH
        rec["checkpoint_s"] = time.time() - t0
        rec["wall_s"] = time.time() - start_time
        rec["sps"] = int(rec["global_step"] / rec["wall_s"])
    return rec["sps"]
