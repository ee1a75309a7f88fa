"""The host harnesses of tests/emul/ have one recipe: every NAME_emul.cpp there has a row in tests/emul/build.sh and builds through
testlib.emul_exe, and the script refuses a name it has no row for."""
import glob
import os
import subprocess

import pytest

from testlib import EMUL_DIR, emul_exe

HARNESSES = sorted(os.path.basename(p)[:-len("_emul.cpp")] for p in glob.glob(os.path.join(EMUL_DIR, "*_emul.cpp")))


def test_there_are_harnesses():
    assert len(HARNESSES) >= 15 and {"walk", "nfa_set_wave_split", "select"} <= set(HARNESSES)


@pytest.mark.parametrize("name", HARNESSES)
def test_every_harness_has_a_row_and_builds(name):
    """(the session's cache of emul_exe makes this cost nothing once another test has built the harness)"""
    exe = emul_exe(name)
    assert os.path.basename(exe) == name + "_emul" and os.access(exe, os.X_OK)


def test_an_unknown_name_is_refused(tmp_path):
    p = subprocess.run([os.path.join(EMUL_DIR, "build.sh"), "no_such_harness", str(tmp_path / "out")], capture_output=True, text=True)
    assert p.returncode == 2 and "no harness named" in p.stderr and not (tmp_path / "out").exists()
