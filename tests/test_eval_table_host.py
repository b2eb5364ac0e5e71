"""The table of ddpm_run's optional evaluations (tasks.EVALS), host side: its order, every parser's key check and plain ints, which
entries params asks for, and that tasks.py itself imports no evaluation module."""
import ast

import numpy as np
import pytest

ORDER = ("bpd", "equivariance", "nearest", "spectrum", "fidelity", "manifold", "restoration")
BASE = {"gen_total": 8, "image_size": 32}
MINIMAL = {"eval_nearest": {"n": np.int64(4)}, "eval_spectrum": {"n": np.int64(4)},
           "eval_fidelity": {"n": np.int64(4), "extractor": "pixels"}, "eval_manifold": {"n": np.int64(4), "extractor": "pixels"},
           "eval_restoration": {"n": np.int64(4)}}


def test_table_order_and_parsers():
    from afdm.tasks import EVALS
    assert tuple(e.out for e in EVALS) == ORDER and tuple(e.key for e in EVALS) == tuple("eval_" + o for o in ORDER)
    assert {e.key for e in EVALS if e.parse is not None} == set(MINIMAL)
    assert [e.out for e in EVALS if e.samples] == ["nearest", "spectrum", "fidelity", "manifold"]
    for e in EVALS:
        if e.parse is None:
            continue
        cfg = e.parse(dict(BASE, **{e.key: MINIMAL[e.key]}))
        assert cfg["n"] == 4 and e.n_min(cfg) <= 4
        for key, val in cfg.items():
            assert not isinstance(val, (bool, np.integer)), (e.key, key)
            if key in ("n", "k", "kid_subsets", "kid_subset_size", "factor"):
                assert type(val) is int, (e.key, key, type(val))
        with pytest.raises(ValueError, match=f"ddpm_run: {e.key} needs n"):
            e.parse(dict(BASE, **{e.key: dict(MINIMAL[e.key], no_such_key=1)}))


def test_asked_evaluations_come_in_table_order():
    from afdm.tasks import _eval_cfgs
    params = dict(BASE, eval_equivariance={"t": 10, "transforms": []}, eval_bpd=2, **dict(reversed(list(MINIMAL.items()))))
    assert [e.out for e in _eval_cfgs(params)] == list(ORDER)
    assert all((cfg is None) == (e.parse is None) for e, cfg in _eval_cfgs(params).items())
    assert _eval_cfgs(dict(BASE, eval_bpd=0, eval_equivariance=None, eval_nearest=None)) == {}
    with pytest.raises(ValueError, match="eval_spectrum needs n"):        # a malformed key fails when the table is parsed
        _eval_cfgs(dict(params, eval_spectrum={}))


def test_tasks_imports_no_evaluation_module_at_import_time():
    import afdm.tasks
    tree = ast.parse(open(afdm.tasks.__file__).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {(n.module or "").split(".")[-1] for n in top if isinstance(n, ast.ImportFrom)}
    names |= {a.name.split(".")[-1] for n in top for a in n.names}
    assert "json" in names and not names & {"fidelity", "manifold", "spectrum", "quality", "imageio_utils"}
