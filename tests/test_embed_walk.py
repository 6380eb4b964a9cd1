"""The group walk both inversion CLIs run (dge_amd.embedding_v2.invert_folder) with a stand-in for the per-group loop: which rows
each group gets, the printed lines, and the files of the walk itself.  The expectations restate the walks that the two main()s
carried separately before they were shared.  Below it the two other host-side pieces the inversion loops share: the iteration
loop (dge_amd.embedding.iterate) on a stub step, and the writer of id{n}-noise.pt (dge_amd.noise_maps.save_noise_rows).  No GPU."""
import os

import pytest
import torch


@pytest.mark.parametrize("independent,labels", [(False, None), (True, None), (True, [30, 207, 5, 1, 9])])
def test_group_walk_of_the_clis(independent, labels, tmp_path, capsys):
    """invert_folder, the walk both main()s run: 5 images at batch 2.  Coupled: the 2 full groups, w1[0] of each, w_all_1.pt.  Rows:
    3 groups, the last padded by its last image (and label) with one row kept, every image's w1, w_all_4.pt."""
    from dge_amd.embedding_v2 import invert_folder
    for sub in ("models", "summaries"):
        os.makedirs(str(tmp_path / sub))
    imgs = torch.arange(5.0).reshape(5, 1, 1, 1).expand(5, 3, 8, 8) / 8
    calls = []

    def invert(imgs1, group, **kw):
        calls.append((imgs1[:, 0, 0, 0].mul(8).int().tolist(), group, kw))
        ev = [(1, 0, 0.5, 1.0)] * (group + 1)
        num = imgs1[:, 0, 0, 0] * 8                                  # row b carries its image number
        return dict(w1=num[:, None] + torch.arange(4.0)[None], imgs2=imgs1, loss_msiv=num / 4 if independent else num[0] / 4,
                    w_norm=num + 0.5 if independent else num[0] + 0.5,
                    tracker=[dict(events=ev)] * imgs1.shape[0] if independent else dict(events=ev))
    invert_folder(invert, imgs, 2, independent, str(tmp_path), labels=labels, save_imgs=labels is not None)
    lines = capsys.readouterr().out.splitlines()
    names = sorted(sub + "/" + n for sub in ("models", "summaries") for n in os.listdir(str(tmp_path / sub)))
    assert sorted(os.listdir(str(tmp_path))) == ["models", "summaries"]
    if not independent:
        assert calls == [([0, 1], 0, {}), ([2, 3], 1, {})]
        assert lines == ["group 0: loss_msiv 0.00000  w_norm 0.5000  events 1", "group 1: loss_msiv 0.50000  w_norm 2.5000  events 2"]
        assert names == ["models/w_all_1.pt", "summaries/00000_rec.png", "summaries/00001_rec.png"]
        assert torch.equal(torch.load(str(tmp_path / "models" / "w_all_1.pt")), torch.tensor([[0.0, 1, 2, 3], [2, 3, 4, 5]]))
        return
    lab = (lambda *ids: {}) if labels is None else (lambda *ids: {"labels": [labels[i] for i in ids]})
    assert calls == [([0, 1], 0, dict(keep=2, **lab(0, 1))), ([2, 3], 1, dict(keep=2, **lab(2, 3))), ([4, 4], 2, dict(keep=1, **lab(4, 4)))]
    tag = [""] * 5 if labels is None else [" (label %d)" % v for v in labels]
    assert lines == ["image %d%s: loss_msiv %.5f  w_norm %.4f  events %d" % (k, tag[k], k / 4, k + 0.5, k // 2 + 1) for k in range(5)]
    assert names == (["models/img_all_4.pt"] if labels is not None else []) + ["models/w_all_4.pt"] + ["summaries/0000%d_rec.png" % g for g in range(3)]
    assert torch.equal(torch.load(str(tmp_path / "models" / "w_all_4.pt")), torch.arange(5.0)[:, None] + torch.arange(4.0)[None])
    if labels is not None:
        assert torch.equal(torch.load(str(tmp_path / "models" / "img_all_4.pt")), imgs)


class _StubStep:
    """What embedding.iterate needs of a step; every call is recorded and stands for one iteration."""

    def __init__(self, captured=False):
        self.captured, self.calls, self.last = captured, [], {"it": "before"}

    def _run(self, what):
        self.calls.append(what)
        self.last = {"it": sum(1 for c in self.calls if c[0] in ("step", "warmup", "replay"))}
        return self.last

    def step(self, imgs1):
        return self._run(("step", imgs1))

    def capture(self, imgs1, warmup):
        self.calls.append(("capture", imgs1, warmup))
        for _ in range(warmup):
            self._run(("warmup",))
        self.captured = True

    def set_image(self, imgs1):
        self.calls.append(("set_image", imgs1))

    def replay(self):
        return self._run(("replay",))


@pytest.mark.parametrize("launch,captured,iterations,indices,calls", [
    ("eager", False, 3, [0, 1, 2], [("step", "img")] * 3),
    ("graph", False, 3, [0, 1, 2], [("capture", "img", 1), ("warmup",), ("replay",), ("replay",)]),
    ("graph", True, 3, [0, 1, 2], [("set_image", "img"), ("replay",), ("replay",), ("replay",)]),
    ("graph", False, 0, [0], [("capture", "img", 1), ("warmup",)]),
])
def test_iterate_runs_each_iteration_once(launch, captured, iterations, indices, calls):
    """embedding.iterate, the loop of invert, invert_group and project: the warm-up iteration of a capture is iteration 0 of the loop
    (also where no iteration was asked for), every other one is a step() or a replay(); the dict yielded with i is iteration i's."""
    from dge_amd.embedding import iterate
    st = _StubStep(captured)
    loop = iterate(st, "img", iterations, launch)
    assert st.calls == []                       # nothing runs before the loop is advanced: the caller's begin_image comes first
    got = list(loop)
    assert [i for i, _ in got] == indices and st.calls == calls
    assert [r["it"] for _, r in got] == [i + 1 for i in indices]


def test_iterate_refuses_an_unknown_launch():
    from dge_amd.embedding import iterate
    st = _StubStep()
    with pytest.raises(ValueError, match="launch must be 'graph' or 'eager', got 'auto'"):
        list(iterate(st, "img", 3, "auto"))
    assert st.calls == []


def test_save_noise_rows_writes_one_list_per_image(tmp_path):
    """noise_maps.save_noise_rows, the one writer of id{n}-noise.pt (embedding_v2.finish_group and projector.project): row b of every
    map, each [1,R,R], under image number n."""
    from dge_amd.noise_maps import save_noise_rows
    maps = [torch.arange(2 * 4 * 4.0).reshape(2, 4, 4), torch.arange(2 * 8 * 8.0).reshape(2, 8, 8) + 100]
    save_noise_rows(maps, (0, 1), (7, 9), str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == ["id7-noise.pt", "id9-noise.pt"]
    for b, n in ((0, 7), (1, 9)):
        got = torch.load(str(tmp_path / ("id%d-noise.pt" % n)))
        assert isinstance(got, list) and [tuple(t.shape) for t in got] == [(1, 4, 4), (1, 8, 8)]
        assert all(torch.equal(t, m[b:b + 1]) for t, m in zip(got, maps))
