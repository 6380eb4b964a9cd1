"""Host-side pieces of the conv launch layer of dge_amd.ops that need neither the library nor a GPU: the low-resolution weight
prefetch chain (CPU tensors have data_ptr() and take weak references), the statistics slot count and the weight image count."""
import gc

import pytest
import torch

from dge_amd import ops

S0, S1 = 0x1000, 0x2000          # two stream handles


def _packed(n=4, k=8):
    return torch.zeros(9, n, k)


def _hint(t):
    return (t.data_ptr(), t.shape[1], t.shape[2])


def test_prefetch_chain_links_the_launch_that_followed_last_time():
    pf, A, B = ops._PrefetchChain(), _packed(4, 8), _packed(16, 32)
    assert pf.link(S0, A) is None and pf.link(S0, B) is None
    assert pf.link(S0, A) == _hint(B)
    assert pf.link(S0, B) == _hint(A)


def test_prefetch_chain_is_keyed_by_stream():
    pf, A, B, X, Y = ops._PrefetchChain(), _packed(), _packed(16, 32), _packed(2, 2), _packed(3, 3)
    got = [pf.link(s, t) for s, t in ((S0, A), (S1, X), (S0, B), (S1, Y), (S0, A), (S1, X))]
    assert got == [None, None, None, None, _hint(B), _hint(Y)]
    assert set(pf.next) == {(S0, A.data_ptr()), (S0, B.data_ptr()), (S1, X.data_ptr()), (S1, Y.data_ptr())}


def test_prefetch_chain_ignores_a_self_link():
    pf, A = ops._PrefetchChain(), _packed()
    assert pf.link(S0, A) is None and pf.link(S0, A) is None
    assert pf.next == {}


def test_prefetch_chain_drops_an_entry_whose_tensor_died():
    pf, A, B = ops._PrefetchChain(), _packed(), _packed(16, 32)
    pf.link(S0, A), pf.link(S0, B)
    assert (S0, A.data_ptr()) in pf.next
    del B
    gc.collect()
    assert pf.link(S0, A) is None
    assert (S0, A.data_ptr()) not in pf.next


def test_prefetch_chain_table_is_cleared_above_512_entries_and_goes_on():
    pf = ops._PrefetchChain()
    ts = [_packed(1, 1) for _ in range(516)]
    sizes = []
    for t in ts:                       # link k (t[k-1] -> t[k]) is recorded by call k: 515 distinct links
        pf.link(S0, t)
        sizes.append(len(pf.next))
    assert sizes[:514] == [0] + list(range(1, 514))     # grows to 513 entries ...
    assert sizes[514:] == [1, 2]                        # ... then one clear, and recording goes on
    A, B = ts[-2], ts[-1]
    assert pf.link(S0, A) == _hint(B) and pf.link(S0, B) == _hint(A)       # (A -> B is the last link recorded above)


def test_prefetch_chain_off_records_nothing():
    pf, A, B = ops._PrefetchChain(on=False), _packed(), _packed(16, 32)
    assert [pf.link(S0, t) for t in (A, B, A)] == [None, None, None]
    assert pf.prev == {} and pf.next == {}


@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (2, 64, 64), (8, 256, 256), (8, 1024, 1024), (3, 100, 36)])
def test_stats_slot_count_matches_the_kernels_tiles(B, H, W):
    assert ops._stats_slots(B, H, W, 16) == max(1, min(64, (((H + 15) // 16) * ((W + 15) // 16) * B) // 16))      # dge_conv2d, in_bwd
    assert ops._stats_slots(B, H, W, 32) == max(1, min(64, (((H + 15) // 16) * ((W + 31) // 32) * B) // 16))      # dge_conv_pp


def test_weight_image_count():
    s3, s5 = torch.zeros(3, 7), torch.zeros(5, 2)
    assert ops._weight_images(None, None) == 1
    assert ops._weight_images(s3, None) == 3 and ops._weight_images(None, s5) == 5
    assert ops._weight_images(s3, s5) == 5              # both given: the last one wins
