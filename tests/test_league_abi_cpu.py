"""CPU-only checks of the league's C-ABI entries (vss_actor_forward_grouped, vss_policy_sample_grouped,
vss_match_tally): every invalid argument is rejected before any HIP call, the ctypes mirror of
vss_actor_groups has the C layout, and pfsp_weights' known answers."""
import ctypes

import pytest

from vss_amd import _native as N

FAKE = 4096  # a non-null, 16-B aligned address that is never dereferenced: every call below is rejected first
E_ARG = 1


def groups(count=4, group_rows=64, actor=FAKE, logstd=FAKE):
    g = N.VssActorGroups()
    g.count, g.group_rows = count, group_rows
    for i in range(N.MAX_ACTOR_GROUPS):
        g.actor_packed[i] = actor
        g.logstd[i] = logstd
    return g


def forward(rows=200, n_act=2, obs=FAKE, g=None, **kw):
    g = groups(**kw) if g is None else g
    return N.load().vss_actor_forward_grouped(None, rows, n_act, obs, ctypes.byref(g) if g else None, 1, 1, FAKE, FAKE)


def sample(rows=200, n_act=2, mean=FAKE, g=None, **kw):
    g = groups(**kw) if g is None else g
    return N.load().vss_policy_sample_grouped(None, rows, n_act, mean, ctypes.byref(g) if g else None, 1, 1, FAKE)


def tally(n_fields=300, rows_per_field=1, group_fields=128, count=3, rew=FAKE, dones=FAKE, progress=FAKE, out=FAKE):
    return N.load().vss_match_tally(None, n_fields, rows_per_field, group_fields, count, rew, dones, progress, out)


def test_struct_mirror_has_the_c_layout():
    assert ctypes.sizeof(N.VssActorGroups) == 4 + 4 + 8 + 16 * 8 + 16 * 8 == 272
    assert N.VssActorGroups.group_rows.offset == 8
    assert N.VssActorGroups.actor_packed.offset == 16
    assert N.VssActorGroups.logstd.offset == 16 + 16 * 8
    assert N.MAX_ACTOR_GROUPS == 16


@pytest.mark.parametrize("call", [forward, sample])
def test_grouped_entries_reject_bad_group_tables(call):
    assert call(count=0) == E_ARG
    assert call(count=17, rows=17 * 64) == E_ARG
    assert call(group_rows=0) == E_ARG
    assert call(group_rows=96, rows=4 * 96) == E_ARG
    assert call(group_rows=-64) == E_ARG
    assert call(rows=4 * 64 + 1) == E_ARG  # rows > count * group_rows
    assert call(rows=3 * 64) == E_ARG  # rows <= (count - 1) * group_rows: the last group would be empty
    assert call(rows=64) == E_ARG
    assert call(rows=-1) == E_ARG
    assert call(n_act=3) == E_ARG
    assert call(g=False) == E_ARG  # a null group pointer
    assert call(logstd=None) == E_ARG


def test_rows_zero_is_ok_without_a_launch():
    assert forward(rows=0) == 0
    assert sample(rows=0) == 0
    assert tally(n_fields=0) == 0
    # the table is still checked
    assert forward(rows=0, count=0) == E_ARG
    assert sample(rows=0, group_rows=96) == E_ARG
    assert tally(n_fields=0, rows_per_field=2) == E_ARG


def test_forward_rejects_null_and_misaligned_pointers():
    assert forward(obs=None) == E_ARG
    assert forward(actor=None) == E_ARG
    assert forward(actor=FAKE + 4) == E_ARG  # packed weights are read as float4
    g = groups()
    g.actor_packed[3] = None  # one used entry
    assert forward(g=g) == E_ARG
    g = groups(count=3, group_rows=64)
    g.actor_packed[3] = None  # entries >= count are unused
    g.logstd[3] = None
    assert forward(rows=0, g=g) == 0


def test_sample_rejects_null_mean_and_ignores_the_packed_weights():
    assert sample(mean=None) == E_ARG
    assert sample(rows=0, actor=None) == 0  # actor_packed is not read and may be null
    assert sample(rows=0, actor=FAKE + 4) == 0


def test_tally_rejects_bad_arguments():
    assert tally(rows_per_field=2) == E_ARG
    assert tally(rows_per_field=0) == E_ARG
    assert tally(count=2) == E_ARG  # count * group_fields = 256 < 300 fields
    assert tally(group_fields=99, count=3) == E_ARG
    assert tally(group_fields=0) == E_ARG
    assert tally(count=0) == E_ARG
    assert tally(count=17) == E_ARG
    assert tally(n_fields=-1) == E_ARG
    assert tally(rew=None) == E_ARG
    assert tally(dones=None) == E_ARG
    assert tally(progress=None) == E_ARG
    assert tally(out=None) == E_ARG
    assert tally(rew=FAKE + 4) == E_ARG  # float4 rows
    assert tally(out=FAKE + 4) == E_ARG  # int64 counters


def test_pfsp_weights_known_answers():
    from vss_amd.opponent import pfsp_weights
    # [episodes, wins, losses, steps]: the learner's win rate 0, 0.5 (by draws and by halves), 1, and unplayed
    totals = [[10, 0, 10, 100], [10, 0, 0, 100], [8, 4, 4, 50], [6, 6, 0, 9], [0, 0, 0, 0]]
    assert pfsp_weights(totals, 1.0) == [1.0, 0.5, 0.5, 0.0, 0.5]
    assert pfsp_weights(totals, 2.0) == [1.0, 0.25, 0.25, 0.0, 0.25]
    import torch
    assert pfsp_weights(torch.tensor(totals), 2.0) == [1.0, 0.25, 0.25, 0.0, 0.25]
    assert pfsp_weights([[4, 1, 1, 7]], 1.0) == [0.5]  # (1 + 0.5 * 2) / 4


def test_an_all_won_pool_is_drawn_uniformly():
    """Every (1 - w) ** power is 0: the weights come back equal, so the draw is uniform."""
    from vss_amd.opponent import pfsp_weights
    assert pfsp_weights([[5, 5, 0, 1], [3, 3, 0, 1], [9, 9, 0, 1]], 1.0) == [1.0, 1.0, 1.0]
    assert pfsp_weights([[5, 5, 0, 1]], 2.0) == [1.0]
