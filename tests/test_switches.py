"""common.switches, the one way the tests set the library's MHH_* environment switches: it restores what was there, through an
exception as well, and refuses a name the library does not read -- KNOWN_SWITCHES is held against the sources."""
import glob
import os
import re

import pytest

import common as cm

NAME = "MHH_PRES_LDS"


def _clean(monkeypatch, value=None):
    if value is None:
        monkeypatch.delenv(NAME, raising=False)
    else:
        monkeypatch.setenv(NAME, value)


@pytest.mark.parametrize("before", [None, "exported"], ids=["absent", "set"])
def test_switches_restore_what_was_there(monkeypatch, before):
    _clean(monkeypatch, before)
    with cm.switches(MHH_PRES_LDS=1):
        assert os.environ[NAME] == "1"                       # str(value)
        with cm.switches(MHH_PRES_LDS="0", MHH_PRES_LDS_KC=3):      # nested, as test_pres2_lds_transform_form does
            assert os.environ[NAME] == "0" and os.environ["MHH_PRES_LDS_KC"] == "3"
        assert os.environ[NAME] == "1" and "MHH_PRES_LDS_KC" not in os.environ
        with cm.switches(MHH_PRES_LDS=None):                 # None: absent for the block
            assert NAME not in os.environ
        assert os.environ[NAME] == "1"
    assert os.environ.get(NAME) == before


@pytest.mark.parametrize("before", [None, "exported"], ids=["absent", "set"])
def test_switches_restore_through_an_exception(monkeypatch, before):
    _clean(monkeypatch, before)
    with pytest.raises(ZeroDivisionError):
        with cm.switches(MHH_PRES_LDS="1"):
            assert os.environ[NAME] == "1"
            1 / 0
    assert os.environ.get(NAME) == before


def test_switches_refuse_an_unknown_name(monkeypatch):
    _clean(monkeypatch)
    with pytest.raises(KeyError, match="MHH_RHS_44_IMPL"):
        with cm.switches(MHH_PRES_LDS="1", MHH_RHS_44_IMPL="cell"):      # MHH_RHS44_IMPL misspelt
            pass
    assert NAME not in os.environ and "MHH_RHS_44_IMPL" not in os.environ     # refused before anything was set
    with pytest.raises(KeyError):
        cm.known_switches({"MASTER_PORT": "1"})


def test_known_switches_are_the_ones_the_sources_read():
    """csrc: every "MHH_..." string literal of a .hip or .h file is the name of an environment variable -- handed to env_is or
    getenv there, or to a helper that does (march_kc's tune name); model.py: the names given to os.environ.get."""
    csrc = os.path.join(cm.ROOT, "microhh_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert files
    found, direct = set(), set()
    for fn in files:
        text = open(fn).read()
        found.update(re.findall(r'"(MHH_[A-Z0-9_]+)"', text))
        direct.update(re.findall(r'\b(?:env_is|getenv)\(\s*"(MHH_[A-Z0-9_]+)"', text))
    assert direct and direct <= found
    model = open(os.path.join(cm.ROOT, "microhh_amd", "model.py")).read()
    py = set(re.findall(r'os\.environ\.get\(\s*"(MHH_[A-Z0-9_]+)"', model))
    assert py
    assert len(set(cm.KNOWN_SWITCHES)) == len(cm.KNOWN_SWITCHES)
    want = found | py
    assert set(cm.KNOWN_SWITCHES) == want, (sorted(want - set(cm.KNOWN_SWITCHES)), sorted(set(cm.KNOWN_SWITCHES) - want))
