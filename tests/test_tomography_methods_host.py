"""The table of reconstruction methods (tomography.RECONSTRUCTIONS) and what is derived from it: the command line's
choices, check_reconstruction's rules and main.run's refusals, with the texts they have always had.  No GPU."""
import argparse
import re

import pytest


def test_command_line_offers_the_tables_methods_and_the_modalities(capsys):
    from paresis_amd import tomography as tomo
    ap = argparse.ArgumentParser()
    tomo.add_tomography_options(ap)
    choices = {a.dest: a.choices for a in ap._actions}
    assert tuple(choices["tomography_method"]) == tuple(tomo.RECONSTRUCTIONS) == ("fbp", "sirt", "cgls", "tv")
    assert tuple(choices["tomography_modality"]) == tomo.MODALITIES == ("attenuation", "phase")
    assert tomo.METHODS + tomo.REGULARISED_METHODS == tuple(tomo.RECONSTRUCTIONS)
    a = ap.parse_args([])
    assert (a.tomography, a.tomography_modality, a.tomography_method, a.tomography_iterations, a.tomography_weight) == \
        (0, "attenuation", "fbp", 0, None)
    for argv in (["--tomography-method", "art"], ["--tomography-modality", "dark"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
        assert "invalid choice" in capsys.readouterr().err


def test_every_method_takes_its_own_options_and_refuses_the_others():
    from paresis_amd import tomography as tomo
    for method, row in tomo.RECONSTRUCTIONS.items():
        own = dict(iterations=3 if row.iterations else None, weight=0.1 if row.weight else None, nonneg=row.nonneg)
        tomo.check_reconstruction(method, **own)
        assert tomo.reconstruct({"sinograms": {}}, method=method, **own) == {}
        refused = [("iterations", None, "method %r needs iterations" % method) if row.iterations else
                   ("iterations", 3, "iterations is an option of the iterative methods (sirt, cgls), not of %s" % method),
                   ("weight", None, "method %r needs weight" % method) if row.weight else
                   ("weight", 0.1, "weight is an option of method 'tv'")]
        if not row.nonneg:
            refused.append(("nonneg", True, "nonneg is an option of method 'sirt'"))
        for option, value, text in refused:
            with pytest.raises(ValueError, match="^%s$" % re.escape(text)):
                tomo.check_reconstruction(method, **dict(own, **{option: value}))


def test_run_refuses_bad_tomography_options_before_anything_else():
    from paresis_amd import _lib, main
    top = _lib.PSX_FBP_MAX_ANGLES
    for options, text in ((dict(tomography=4, tomography_modality="dark"), "tomography_modality must be one of attenuation, phase, got 'dark'"),
                          (dict(tomography_modality="phase"), "tomography_modality is an option of tomography"),
                          (dict(tomography=-1), "tomography takes 1 to %d angles, got -1" % top),
                          (dict(tomography=top + 1), "tomography takes 1 to %d angles, got %d" % (top, top + 1)),
                          (dict(tomography=4, tomography_method="art"), "method must be one of fbp, sirt, cgls, tv, got 'art'")):
        with pytest.raises(ValueError, match="^%s$" % re.escape(text)):
            main.run({"nbExpPoints": 1}, save=False, **options)
