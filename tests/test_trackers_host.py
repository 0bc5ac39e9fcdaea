"""The one description of the four speckle trackers (retrieval.TRACKERS, ops._tracker_args) without a GPU: the table against
what the ops functions document, the method names both command lines take, and the order in which each ops function's
argument checks fire."""
import argparse
import re

import pytest
import torch

from paresis_amd import main, ops, retrieval
from paresis_amd._lib import PsxError

WORDS = {"three": 3, "four": 4, "five": 5}


def test_table_against_save_order_and_ops():
    assert retrieval.METHODS == ("lcs", "umpa", "umpa-df")
    assert retrieval.UMPA_METHODS == ("umpa", "umpa-df")
    assert sorted(retrieval.TRACKERS) == [('lcs', False), ('lcs', True), ('umpa', False), ('umpa-df', False)]
    counts = []
    for t in retrieval.TRACKERS.values():
        assert set(t.maps) <= set(retrieval.MAP_ORDER) and len(set(t.maps)) == len(t.maps)
        said = re.search(r"out: (\w+)\s+caller-owned", getattr(ops, t.op).__doc__).group(1)      # "out: four caller-owned ..."
        assert len(t.maps) == WORDS[said] and ops._COUNT_WORDS[len(t.maps)] == said
        counts.append(len(t.maps))
    assert counts == [3, 4, 4, 5]
    assert [t.min_positions for t in retrieval.TRACKERS.values()] == [3, 4, 1, 1]


@pytest.mark.parametrize("which", ["main", "retrieval"])
def test_both_parsers_take_the_methods_and_no_other(which, tmp_path, capsys):
    ap = argparse.ArgumentParser()
    retrieval.add_retrieval_options(ap)
    for m in retrieval.METHODS:
        assert ap.parse_args(["--method", m]).method == m
    cli = ((lambda a: main.main(["--retrieve", "--out", str(tmp_path)] + a)) if which == "main"
           else (lambda a: retrieval.main([str(tmp_path)] + a)))
    for m in ("lcs-df", "xst"):
        with pytest.raises(SystemExit) as e:
            cli(["--method", m])
        assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    # each accepted name gets past the parser: main.py stops at its own --points rule, the retrieval CLI at the empty directory
    for m in retrieval.METHODS:
        if which == "main":
            with pytest.raises(SystemExit) as e:
                cli(["--method", m, "--points", "0"])
            assert e.value.code == 2 and "--retrieve needs --points" in capsys.readouterr().err
        else:
            with pytest.raises(ValueError, match="no sample/ and ref/"):
                cli(["--method", m])


def _img(K, n=16, m=16):
    return torch.ones((K, n, m), dtype=torch.float32)


TRACKER_CALLS = [(ops.lcs, 3, {}), (ops.lcs_df, 4, {}), (ops.umpa, 1, {}), (ops.umpa_df, 1, {})]


@pytest.mark.parametrize("fn,kmin,kw", TRACKER_CALLS, ids=[c[0].__name__ for c in TRACKER_CALLS])
def test_error_precedence(fn, kmin, kw):
    """Every input below is wrong in all the later ways too (CPU tensors throughout: the HBM check is the last to fire): the K
    range, then (UMPA) "integer in", then "smaller than", then "positions", then (umpa_df) the means and the number of out=
    tensors, then "shape", then "HBM"."""
    umpa = fn in (ops.umpa, ops.umpa_df)
    K = kmin + 1
    bad_ws = {'window': 0} if umpa else {}
    small = (10, 16) if umpa else (2, 16)                   # below 2*(2+3)+1 = 11, below 3
    with pytest.raises(PsxError, match=r"sample: K=%d positions outside \[%d, 64\]" % (kmin - 1, kmin)):
        fn(_img(kmin - 1, *small), _img(K, 16, 17), **bad_ws)
    with pytest.raises(PsxError, match=r"reference: K=65 positions outside"):
        fn(_img(K, *small), _img(65, 16, 17), **bad_ws)
    if umpa:
        with pytest.raises(PsxError, match="window must be an integer in"):
            fn(_img(K, *small), _img(K + 1, 16, 17), window=0)
        with pytest.raises(PsxError, match="smaller than 11x11"):
            fn(_img(K, *small), _img(K + 1, 16, 17))
    with pytest.raises(PsxError, match="sample has %d positions, reference %d" % (K, K + 1)):
        fn(_img(K), _img(K + 1, 16, 17), **({'mean': [float('nan')]} if fn is ops.umpa_df else {}))
    if fn is ops.umpa_df:
        with pytest.raises(PsxError, match="mean must hold one value per position"):
            fn(_img(K), _img(K, 16, 17), mean=[1.0], out=[torch.empty(16, 16)] * 4)
        with pytest.raises(PsxError, match="out must hold five tensors"):
            fn(_img(K), _img(K, 16, 17), mean=[1.0] * K, out=[torch.empty(16, 16)] * 4)
    with pytest.raises(PsxError, match="reference images have shape"):
        fn(_img(K), _img(K, 16, 17), out=[torch.empty(16, 16)] * 2 if fn is not ops.umpa_df else None)
    if not umpa:
        with pytest.raises(PsxError, match="smaller than 3x3"):
            fn(_img(K, *small), _img(K, *small), max_shift=-1.0)
    with pytest.raises(PsxError, match="HBM"):
        fn(_img(K), _img(K), out=[torch.empty(16, 16)] * 2 if fn is not ops.umpa_df else None,
           **({} if umpa else {'max_shift': -1.0}))
