"""What the perception, the actuation, the estimation and the tracking channel (perceive.py, actuate.py, estimate.py,
track.py) share on the kernel's side: where a layout's units lie, the checks on the buffers a call is handed, and the checkpoint entries.

A layout is a NamedTuple that begins (field_stride, team_stride, robots, n_teams); a unit is what its strides count:
a 52-float observation row, or a robot's two command floats."""
from __future__ import annotations

import numpy as np
import torch

from .checkpoint import copy_entries, entry, to_cpu


def span(layout, n_fields: int) -> int:
    """Units from the layout's first one to the last one's end."""
    return (layout.n_teams - 1) * layout.team_stride + max(n_fields - 1, 0) * layout.field_stride + layout.robots


def index(layout, n_fields: int) -> np.ndarray:
    """(n_teams, n_fields, robots) int64: the unit of team block b, field f, robot k."""
    b = np.arange(layout.n_teams, dtype=np.int64)[:, None, None]
    f = np.arange(n_fields, dtype=np.int64)[None, :, None]
    k = np.arange(layout.robots, dtype=np.int64)[None, None, :]
    return b * layout.team_stride + f * layout.field_stride + k


class Channel:
    """The base of the four channel classes.  A subclass sets device, n_fields, layout and done_stride, calls
    _set_rows(), and names its device tensors in _state_tensors(); the checkpoint label is the class's name.
    (setplay.Stager and referee.Referee have no layout of their own -- their views come with every call -- and use the
    checkpoint half.)"""
    unit = "rows"            # what the layout counts, for the messages
    width = 52               # floats per unit
    scalars = {"call": int}  # the state_dict entries that are not tensors: attribute -> type

    def _set_rows(self, rows: int | None) -> None:
        need = self.layout.span(self.n_fields)
        self.rows = need if rows is None else int(rows)
        if self.rows < need:
            raise ValueError(f"the layout spans {need} {self.unit}, the buffers have {self.rows}")
        self._where = torch.empty(0, device=self.device).device  # the buffers' device, with its index

    def _check_rows(self, t: torch.Tensor, name: str) -> None:
        if (t.dtype != torch.float32 or t.device != self._where or not t.is_contiguous()
                or t.numel() != self.rows * self.width):
            raise ValueError(f"{name} must be {self.rows} contiguous float32 rows of {self.width} on {self._where}, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")

    def _done_ok(self, done) -> bool:
        need = (self.n_fields - 1) * self.done_stride + 1 if self.n_fields else 0
        return (done is not None and done.dtype == torch.long and done.device == self._where and done.is_contiguous()
                and done.numel() >= need)

    def _check_done(self, done: torch.Tensor) -> None:
        if not self._done_ok(done):
            raise ValueError(f"done must be contiguous int64 with a flag every {self.done_stride} elements for "
                             f"{self.n_fields} fields, got {tuple(done.shape)} {done.dtype}")

    def state_dict(self) -> dict:
        """The device tensors (the outputs, the next rollout's first input, among them) on the CPU, and the scalars."""
        return dict(to_cpu(self._state_tensors()), **{k: kind(getattr(self, k)) for k, kind in self.scalars.items()})

    def load_state_dict(self, state: dict) -> None:
        label = type(self).__name__
        copy_entries(label, self._state_tensors(), state)
        for k, kind in self.scalars.items():
            setattr(self, k, kind(entry(state, k, label)))
