"""dge_amd.embed_track.EmbedTracker on the host: buffer identity across groups (a captured iteration reads these buffers), the three
regimes of the minima, and the ring read-out.  reset() and read() need no library, so this runs on CPU tensors."""
import pytest
import torch

from dge_amd.embed_track import EVENT_LOSS, EVENT_NORM, EmbedTracker, tracker_rules

STATE = ("istate", "fstate", "best_loss", "best_norm", "events", "l2")


def ptrs(t):
    return [getattr(t, k).data_ptr() for k in STATE]


@pytest.mark.parametrize("rows", [False, True])
def test_buffers_keep_their_address_until_the_latent_shape_changes(rows):
    t = EmbedTracker(tracker_rules("sg2", 2001), events_cap=8, rows=rows)
    t.reset((2, 9, 512), "cpu")
    lead = (2,) if rows else ()
    assert [tuple(getattr(t, k).shape) for k in STATE] == [lead + (4,), lead + (2,), (2, 9, 512), (2, 9, 512), lead + (8, 4), lead]
    assert t.istate.dtype == torch.int32 and all(getattr(t, k).dtype == torch.float32 for k in STATE[1:])
    first = ptrs(t)
    t.istate.fill_(3)
    t.events.fill_(1.0)
    t.reset((2, 9, 512), torch.device("cpu"))
    assert ptrs(t) == first                                        # same shape: every tensor stays where it is ...
    assert not t.istate.any() and not t.events.any()               # ... and the counters and the ring restart in place
    keep = [getattr(t, k) for k in STATE]                          # (hold the old tensors: their addresses cannot be handed out again)
    t.reset((3, 9, 512), "cpu")                                    # another B
    assert tuple(t.best_loss.shape) == (3, 9, 512) and not set(ptrs(t)) & set(first)
    second = ptrs(t)
    keep += [getattr(t, k) for k in STATE]
    t.reset((1, 27, 512), "cpu")                                   # another shape with the same number of elements
    assert tuple(t.best_norm.shape) == (1, 27, 512) and not set(ptrs(t)) & set(second)
    assert tuple(t.fstate.shape) == ((1, 2) if rows else (2,))
    del keep


def test_equal_element_count_is_not_equal_shape():
    t = EmbedTracker(tracker_rules("sg2", 2001), events_cap=4, rows=True)
    t.reset((2, 9, 512), "cpu")
    old = [getattr(t, k) for k in STATE]
    t.reset((1, 18, 512), "cpu")
    assert tuple(t.istate.shape) == (1, 4) and tuple(t.best_loss.shape) == (1, 18, 512) and tuple(t.l2.shape) == (1,)
    assert all(getattr(t, k) is not o for k, o in zip(STATE, old))


def test_sg1_minima_restart_with_every_group():
    rules = tracker_rules("sg1", 1501)
    assert rules["init"] == (0.0, 0.0) and rules["reset_per_group"]
    t = EmbedTracker(rules, events_cap=4)
    t.reset((1, 128), "cpu")
    assert t.fstate.tolist() == [0.0, 0.0]
    t.fstate.copy_(torch.tensor([0.25, 7.0]))
    t.reset((1, 128), "cpu")
    assert t.fstate.tolist() == [0.0, 0.0]


def test_sg2_coupled_minima_carry_over_between_groups():
    rules = tracker_rules("sg2", 2001)
    assert rules["init"] == (100.0, 1000.0) and not rules["reset_per_group"]
    t = EmbedTracker(rules, events_cap=4)
    t.reset((1, 18, 512), "cpu")
    assert t.fstate.tolist() == [100.0, 1000.0]                    # a fresh allocation starts from init
    t.fstate.copy_(torch.tensor([0.25, 7.0]))
    t.reset((1, 18, 512), "cpu")
    assert t.fstate.tolist() == [0.25, 7.0]                        # the next group inherits the minima
    t.reset((2, 18, 512), "cpu")
    assert t.fstate.tolist() == [100.0, 1000.0]                    # a new allocation starts from init again


def test_sg2_rows_minima_restart_with_every_group():
    t = EmbedTracker(tracker_rules("sg2", 2001), events_cap=4, rows=True)
    t.reset((3, 18, 512), "cpu")
    assert t.fstate.tolist() == [[100.0, 1000.0]] * 3
    t.fstate.copy_(torch.tensor([[0.25, 7.0], [0.5, 8.0], [0.75, 9.0]]))
    t.reset((3, 18, 512), "cpu")
    assert t.fstate.tolist() == [[100.0, 1000.0]] * 3


def slots(base):
    """Four ring slots (iteration, kind, loss, norm); slot s holds iteration base + s."""
    return torch.tensor([[base + s, (EVENT_LOSS, EVENT_NORM)[s % 2], 0.5 + s, 2.0 * s + base] for s in range(4)], dtype=torch.float32)


def events_of(base, order):
    return [(base + s, (EVENT_LOSS, EVENT_NORM)[s % 2], 0.5 + s, 2.0 * s + base) for s in order]


def test_ring_read_out_is_oldest_first():
    t = EmbedTracker(tracker_rules("sg2", 2001), events_cap=4)
    t.reset((2, 3), "cpu")
    t.istate.copy_(torch.tensor([7, 6, 2, 1], dtype=torch.int32))          # 6 events written into 4 slots: 2 dropped, next slot 6 % 4
    t.fstate.copy_(torch.tensor([0.125, 3.5]))
    t.events.copy_(slots(10))
    t.best_loss.copy_(torch.arange(6.0).reshape(2, 3))
    t.best_norm.copy_(torch.arange(6.0).reshape(2, 3) + 10)
    tr = t.read()
    assert sorted(tr) == ["best_loss", "best_norm", "dropped", "events", "iteration", "min_loss", "min_norm"]
    assert (tr["iteration"], tr["dropped"], tr["min_loss"], tr["min_norm"]) == (7, 2, 0.125, 3.5)
    assert all(type(tr[k]) is int for k in ("iteration", "dropped")) and all(type(tr[k]) is float for k in ("min_loss", "min_norm"))
    assert tr["events"] == events_of(10, [2, 3, 0, 1])
    assert all(type(e[0]) is int and type(e[1]) is int and type(e[2]) is float and type(e[3]) is float for e in tr["events"])
    assert torch.equal(tr["best_loss"], torch.arange(6.0).reshape(2, 3)) and torch.equal(tr["best_norm"], torch.arange(6.0).reshape(2, 3) + 10)
    assert tr["best_loss"].data_ptr() != t.best_loss.data_ptr() and tr["best_norm"].data_ptr() != t.best_norm.data_ptr()


def test_ring_read_out_of_rows_with_their_own_counts():
    t = EmbedTracker(tracker_rules("sg2", 2001), events_cap=4, rows=True)
    t.reset((2, 3, 5), "cpu")
    t.istate.copy_(torch.tensor([[7, 6, 2, 1], [9, 3, 0, 1]], dtype=torch.int32))      # row 0 wrapped, row 1 holds 3 events
    t.fstate.copy_(torch.tensor([[0.125, 3.5], [0.25, 4.5]]))
    t.events.copy_(torch.stack((slots(10), slots(20))))
    t.best_loss.copy_(torch.arange(30.0).reshape(2, 3, 5))
    t.best_norm.copy_(torch.arange(30.0).reshape(2, 3, 5) + 100)
    trs = t.read()
    assert isinstance(trs, list) and len(trs) == 2
    assert (trs[0]["iteration"], trs[0]["dropped"], trs[0]["min_loss"], trs[0]["min_norm"]) == (7, 2, 0.125, 3.5)
    assert (trs[1]["iteration"], trs[1]["dropped"], trs[1]["min_loss"], trs[1]["min_norm"]) == (9, 0, 0.25, 4.5)
    assert trs[0]["events"] == events_of(10, [2, 3, 0, 1])
    assert trs[1]["events"] == events_of(20, [0, 1, 2])
    for b, tr in enumerate(trs):
        assert tuple(tr["best_loss"].shape) == (1, 3, 5) and tuple(tr["best_norm"].shape) == (1, 3, 5)
        assert torch.equal(tr["best_loss"], torch.arange(30.0).reshape(2, 3, 5)[b:b + 1])
        assert torch.equal(tr["best_norm"], torch.arange(30.0).reshape(2, 3, 5)[b:b + 1] + 100)
    t.best_loss.fill_(-1.0)                                              # a clone, not a view of the device state
    t.best_norm.fill_(-1.0)
    assert float(trs[1]["best_loss"][0, 0, 0]) == 15.0 and float(trs[1]["best_norm"][0, 0, 0]) == 115.0
    assert trs[0]["best_loss"].data_ptr() != t.best_loss.data_ptr()


class _StubEncoder:
    """What LatentEmbedStep's constructor needs of a frozen encoder."""
    layer_count = 5

    def parameters(self):
        return []

    def eval(self):
        return self


def test_the_steps_hold_one_tracker_that_shares_their_rules():
    from dge_amd.embedding_v2 import LatentEmbedStep
    st = LatentEmbedStep(None, _StubEncoder(), None, mode="W", generator="sg2", arm_iter=3, events_cap=16, independent=True)
    assert isinstance(st._tracker, EmbedTracker) and st._tracker.rules is st.rules and st.rules["arm_iter"] == 3
    assert st._tracker.rows and st._tracker.cap == 16
    with pytest.raises(RuntimeError, match="begin_image"):
        st.step(torch.zeros(1, 3, 8, 8))
