"""The cases of tests/test_gpu_param_grads.py are fair: with plain CPU fp32 torch in the kernels' place every one of them passes
the gates the GPU test uses (rel-L2 < 1e-5 against fp64 of what was ADDED to a pre-filled gradient, and of every activation
gradient), so a gate missed on the device is the kernel's fault.  Also here, because they need no device: the layout of the
flat buffers (spacers, sentinels, the pointer offsets every op gets to see) and the two pure functions behind the
tied-parameter rule of ops.inplace_param_grads -- fold_batches (no gradient twice in one fold launch) and deal_lane (every
writer of a gradient on its first writer's side stream)."""
import struct

import pytest
import torch

import param_grad_cases as PG

NAMES = list(PG.all_cases())


def test_layout_spacers_and_offsets():
    lay = PG.Layout({"a": (4,), "b": (4, 4), "c": (3,), "d": (7,), "e": (2, 2)}, rot=0)
    end = lay.head
    for name, (o, n, shape) in lay.slots.items():
        assert 1 <= o - end <= 3, (name, o, end)                       # a spacer of 1, 2 or 3 floats before every tensor
        end = o + n
    assert lay.numel == end + PG.TAIL
    assert [lay.residue(k) for k in "abcd"] == [4, 8, 12, 0]
    flat = lay.fill({k: torch.zeros(s) for k, (_, _, s) in lay.slots.items()})
    assert lay.sentinels_intact(flat) and int(lay.spacers().sum()) == lay.numel - (4 + 16 + 3 + 7 + 4)
    assert bool((flat[lay.spacers()] == PG.SENTINEL).all()) and not flat[~lay.spacers()].any()
    for i in torch.nonzero(lay.spacers()).flatten().tolist():          # every single spacer float is watched
        bad = flat.clone()
        bad[i] = 7.2500005
        assert not lay.sentinels_intact(bad)
    first = PG.Layout({"a": (9,), "b": (2,)}, rot=3)                   # the first tensor as the aligned control
    assert first.head == 1 and first.slots["a"][0] == 4 and first.residue("a") == 0 and lay.head == 0
    v = lay.view(flat, "b")
    assert v.shape == (4, 4) and v.data_ptr() == flat.data_ptr() + 4 * lay.slots["b"][0]


def test_every_op_sees_all_four_pointer_offsets():
    """over the cases of an op, its parameters (= their gradients: same layout) sit 4, 8 and 12 bytes past a 16-byte
    boundary, and on one"""
    seen = {}
    for c in PG.all_cases().values():
        seen.setdefault(c.family, set()).update(c.layout.residue(k) for k in c.params)
    for fam, s in seen.items():
        assert s == {0, 4, 8, 12}, (fam, s)
    # the output layer's odd-sized pair (96 + 3 floats) and the one-tensor ops at more than one offset among their cases
    oc = [c for n, c in PG.all_cases().items() if "output layer" in n]
    assert {c.layout.slots["w"][1] for c in oc} == {96} and {c.layout.slots["b"][1] for c in oc} == {3}
    assert len({(c.layout.residue("w"), c.layout.residue("b")) for c in oc}) == 2


@pytest.mark.parametrize("name", NAMES)
def test_case_passes_in_fp32(name):
    """plain fp32 on the CPU under the GPU test's gates: got = g0 + gradient (one fp32 add, as the kernels' accumulate)"""
    c = PG.all_cases()[name]
    outs64, g64 = c.ref
    outs32, g32 = c.run(torch.float32)
    for o32, o64 in zip(outs32, outs64):
        assert torch.isfinite(o32).all() and PG.rel_l2(o32, o64) < PG.TOL, name
    for k in c.params:
        assert float(g64[k].norm()) > 0 and torch.isfinite(c.g0[k]).all()
        got = c.g0[k] + g32[k]
        assert PG.rel_l2(PG.accumulated(got, c.g0[k]), g64[k]) < PG.TOL, (name, k)
        assert PG.rel_l2(PG.accumulated(g32[k], c.g0[k]), g64[k]) > 0.5, (name, k)       # `=` for `+=` cannot pass: g0 is as large as the gradient
    for k in c.acts:
        assert PG.rel_l2(g32[k], g64[k]) < PG.TOL, (name, k)


def test_tied_reference_is_the_sum_of_both_uses():
    c = PG.all_cases()["tied conv1x1 bias 32to32 8x8"]
    w, b, x = (t.double() for t in (c.params["w"], c.params["b"], c.acts["x"]))
    w1, w2 = w.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, w1, b), w2, b)
    g1, g2 = torch.autograd.grad(y, [w1, w2], c.dys[0].double())
    assert PG.rel_l2(g1 + g2, c.ref[1]["w"]) < 1e-14 and PG.rel_l2(g2, c.ref[1]["w"]) > 0.1


def test_configs():
    assert PG.CONFIGS[0][0] == 0 and {(s, fe) for s, fe, _ in PG.CONFIGS} == {(0, 2), (1, 0), (1, 1), (1, 2), (2, 2)}
    assert {b for _, _, b in PG.CONFIGS} == {1, 8} and len(PG.CONFIGS) == 9


# ---- the tied-parameter rule of ops.inplace_param_grads ---------------------------------------------------------------------
def _ops():
    from afdm import ops
    return ops


def _desc(ops, dst, part=0x1000, n=64):
    return ops.fold_desc(part, dst, n, 3)


def _dsts(batch):
    return [struct.unpack_from("<Q", batch, o + 8)[0] for o in range(0, len(batch), 56)]


def _one_launch_is_safe(batches):
    return all(len(set(_dsts(b))) == len(_dsts(b)) and len(_dsts(b)) <= 56 for b in batches)


def test_fold_batches_never_puts_a_gradient_twice_into_one_launch():
    """fold_batched_k reads dst, adds, writes back, without atomics: two descriptors with one dst in one launch race.  What
    the parent commit did -- every queued descriptor of a stream in ONE launch -- is the `[packed]` below, and it is unsafe
    for every input here that repeats a dst."""
    ops = _ops()
    d = lambda dst, part=0x1000: _desc(ops, dst, part)
    # no repeats: one batch, the very bytes, order kept
    plain = b"".join(d(0x100 * (i + 1)) for i in range(10))
    assert ops.fold_batches(plain) == [plain] and _one_launch_is_safe([plain])
    # a repeated dst: the second starts a new launch; order kept, nothing lost
    a, b, c, a2 = d(0xA00, 0x1000), d(0xB00), d(0xC00), d(0xA00, 0x2000)
    packed = a + b + a2 + c
    got = ops.fold_batches(packed)
    assert got == [a + b, a2 + c] and b"".join(got) == packed
    assert _one_launch_is_safe(got) and not _one_launch_is_safe([packed])            # the parent's single launch
    # a weight and bias pair folded twice (a module called twice): (w, b), (w, b)
    w1, b1, w2, b2 = d(0xA00, 0x1000), d(0xB00, 0x1100), d(0xA00, 0x2000), d(0xB00, 0x2100)
    assert ops.fold_batches(w1 + b1 + w2 + b2) == [w1 + b1, w2 + b2]
    # three times: three launches
    a3 = d(0xA00, 0x3000)
    got = ops.fold_batches(a + a2 + b + a3 + c)
    assert got == [a, a2 + b, a3 + c] and _one_launch_is_safe(got) and not _one_launch_is_safe([a + a2 + b + a3 + c])
    # more than 56 descriptors: the cuts fold_launch makes by itself (kFoldMax), so nothing changes for a model without repeats
    many = [d(0x100 * (i + 1)) for i in range(130)]
    got = ops.fold_batches(b"".join(many))
    assert [len(g) // 56 for g in got] == [56, 56, 18] and b"".join(got) == b"".join(many)
    # ... and a repeat behind such a cut, or far apart inside one
    many[100] = d(0x100 * 61, 0x9000)                                                # dst of descriptor 60, same launch (56..111)
    got = ops.fold_batches(b"".join(many))
    assert b"".join(got) == b"".join(many) and _one_launch_is_safe(got) and [len(g) // 56 for g in got] == [56, 44, 30]
    assert ops.FOLD_MAX == 56 and struct.calcsize(ops.FOLD_DESC) == 56


def test_deal_lane_keeps_every_writer_of_a_gradient_on_one_stream():
    ops = _ops()
    # no repeats: plain round-robin, as the parent dealt them
    lane_of, lanes = {}, []
    for turn, keys in enumerate([[1, 2], [3, 4], [5], [6, 7], [8]]):
        lanes.append(ops.deal_lane(keys, lane_of, turn, 2))
    assert lanes == [(0, False), (1, False), (0, False), (1, False), (0, False)]
    # one side stream: always lane 0
    assert [ops.deal_lane([k], {}, t, 1) for t, k in enumerate((1, 1, 2))] == [(0, False)] * 3
    # a module called twice: its second use falls on the OTHER lane by round-robin (the parent's race) and is pulled back
    lane_of = {}
    got = [ops.deal_lane(keys, lane_of, turn, 2) for turn, keys in enumerate([[1, 2], [1, 2], [3], [1, 2], [3]])]
    assert got == [(0, False), (0, False), (0, False), (0, False), (0, False)] and [t % 2 for t in range(5)] != [g[0] for g in got]
    lane_of = {}
    got = [ops.deal_lane(keys, lane_of, turn, 2) for turn, keys in enumerate([[9], [1, 2], [3], [1, 2]])]
    assert got == [(0, False), (1, False), (0, False), (1, False)]
    # gradients that already live on different lanes: reported, so that the caller orders the lanes first
    lane_of = {}
    assert ops.deal_lane([1, 2], lane_of, 0, 2) == (0, False) and ops.deal_lane([3, 4], lane_of, 1, 2) == (1, False)
    assert ops.deal_lane([1, 4], lane_of, 2, 2) == (0, True) and lane_of[4] == 0
