"""The C-ABI called from C: integration/capi_smoke.c includes include/mfa_hip.h under `cc -std=c11 -Wall -Wextra -Werror -pedantic`
(the header is C, not C++), links libmfa_hip.so, loads a fixture blob, matches a golden string set with one
mfa_match_batch_host call and compares with the reference's answers.  What a maintainer of matchers/match.cpp:21-31 would link."""
import os
import subprocess

import pytest

import oracle_lib
from mfa_amd import image
from testlib import CSRC


@pytest.fixture(scope="module")
def smoke(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("capi_c") / "capi_smoke")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(oracle_lib.ROOT, "include"), "-o", out,
                           os.path.join(oracle_lib.ROOT, "integration", "capi_smoke.c"), "-L" + CSRC, "-lmfa_hip", "-Wl,-rpath," + CSRC])
    return out


def blob_file(tmp_path, name):
    p = tmp_path / (name + ".blob")
    p.write_bytes(bytes(image.blob_from_dump(oracle_lib.load_dump(name))))
    return str(p)


def test_header_is_c_and_no_device_is_an_error(smoke, tmp_path):
    """Builds as strict C11; without a GPU the match call reports MFA_ERR_NO_DEVICE through the C caller (exit code 3), never an answer."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the run is checked by test_c_caller_matches_goldens")
    p = subprocess.run([smoke, blob_file(tmp_path, "ex1_plain"), os.path.join(oracle_lib.GOLDEN, "strings", "abc7.txt"),
                        os.path.join(oracle_lib.GOLDEN, "results", "ex1_plain.abc7.bits")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 3 and "no usable HIP device" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,sset", [("ex1_plain", "abc7"), ("ex8_reverse", "pump8"), ("ex3_bnf", "rnd"), ("nfa_abb_thompson", "abc7")])
def test_c_caller_matches_goldens(smoke, tmp_path, name, sset):
    p = subprocess.run([smoke, blob_file(tmp_path, name), os.path.join(oracle_lib.GOLDEN, "strings", sset + ".txt"),
                        os.path.join(oracle_lib.GOLDEN, "results", "%s.%s.bits" % (name, sset))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 differences" in p.stdout
