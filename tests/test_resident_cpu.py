"""CPU tier of the resident scope (include/parasuite_hip.h: ps_resident_begin / _end / _info).

* The books of the scope (csrc/ps_resident.h: keys, the identity of the index files, the LRU bound, drop-after-error, the end of a
  scope, who holds a device's lanes of work) are driven by tests/resident_check.cpp with stub payloads and stub closers -- a plain
  executable built here with the host compiler, AddressSanitizer and UBSan; it checks itself and prints one `ok` line per part.
* Through the library, which loads without a GPU: the error cases of begin and end, struct_size, ps_resident_info before any
  scope (in a fresh process) and after one, and capi.resident ending its scope when its body raises."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from test_capi_cpu import ROOT

CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
COUNTERS = ("n_calls", "n_index_loads", "n_index_reuses", "n_stale_reloads", "n_evictions", "n_dropped_after_error")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resident") / "resident_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "resident_check.cpp"), "-o", out])
    return out


def _ok(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["ok " + " ".join(str(a) for a in args if not os.path.isdir(str(a)))], r.stdout


def test_the_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ps_resident.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and not any("hip/" in i for i in includes), includes
    assert [i for i in includes if i.startswith('"')] == ['"../../include/parasuite_hip.h"', '"ps_map_plan.h"']


def test_keys(exe, tmp_path):
    """the path spelled several ways, device plan 0 against 0,0, each knob (PS_JUMP_LEVELS among them)"""
    _ok(exe, "keys", tmp_path)


def test_identity_change_in_each_field_is_stale(exe, tmp_path):
    _ok(exe, "identity", tmp_path)


@pytest.mark.parametrize("max_references", [1, 2, 8])
def test_lru_order_and_eviction(exe, max_references):
    _ok(exe, "lru", max_references)


def test_drop_after_error_invalidate_and_end(exe):
    """exactly the entries a failed call used go; every closer ran once, before the operation returned; end closes all"""
    _ok(exe, "drop_and_end")


def test_never_two_lane_owners_per_device(exe):
    _ok(exe, "lanes")


def test_opts_struct(exe):
    _ok(exe, "opts")


# ---- through the library --------------------------------------------------------------------------------------------------------
@pytest.fixture
def closed_scope():
    """the process has one scope: whatever a test leaves open is ended, so that the tests after it start outside a scope"""
    import capi
    assert capi.ps_resident_info()["active"] == 0
    yield capi
    if capi.ps_resident_info()["active"]:
        capi.ps_resident_end()


def test_info_before_any_scope():
    """a fresh process: nothing is active and every counter is zero; asking makes no device call and needs none"""
    code = ("import sys; sys.path.insert(0, %r); import capi; i = capi.ps_resident_info(); "
            "assert set(i) == {'active', 'n_references', 'bytes_index_resident'} | set(%r), i; assert not any(i.values()), i; print('fresh ok')"
            % (os.path.join(ROOT, "para-suite_amd"), COUNTERS))
    out = subprocess.run([sys.executable, "-c", code], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("fresh ok"), out.stdout


def test_begin_and_end_error_cases(closed_scope):
    capi = closed_scope
    L = capi.lib()
    assert L.ps_resident_end() == 1 and b"no scope is open" in L.ps_last_error()
    assert L.ps_resident_begin(None) == 0                             # NULL: the defaults
    i = capi.ps_resident_info()
    assert i["active"] == 1 and i["n_references"] == 0 and i["bytes_index_resident"] == 0 and not any(i[k] for k in COUNTERS)
    assert L.ps_resident_begin(None) == 1 and b"open already" in L.ps_last_error()
    assert capi.ps_resident_info()["active"] == 1                      # the refused begin changed nothing
    assert L.ps_resident_end() == 0
    assert capi.ps_resident_info()["active"] == 0
    assert L.ps_resident_end() == 1 and b"no scope is open" in L.ps_last_error()
    for bad in (0, 9, 2 ** 32 - 1):
        with pytest.raises(capi.PsError, match=r"max_references is %d, accepted: 1 to 8" % bad):
            capi.ps_resident_begin(bad)
        assert capi.ps_resident_info()["active"] == 0
    for ok in (1, 8):
        capi.ps_resident_begin(ok)
        capi.ps_resident_end()
    assert L.ps_resident_info(None) == 1 and L.ps_last_error()


def test_struct_size(closed_scope):
    capi = closed_scope
    L = capi.lib()
    o = capi.ResidentOpts(4, 99)                                       # a caller whose struct ends before max_references: the default, 99 is not read
    assert L.ps_resident_begin(C.byref(o)) == 0 and L.ps_resident_end() == 0
    for bad in (0, 2, 6, 12, 64):                                      # no multiple of 4, or longer than this library knows
        o = capi.ResidentOpts(bad, 2)
        assert L.ps_resident_begin(C.byref(o)) == 1, bad
        msg = L.ps_last_error()
        assert b"ps_resident_opts" in msg and b"struct_size" in msg and str(bad).encode() in msg, msg
        assert capi.ps_resident_info()["active"] == 0


def test_context_manager_ends_the_scope_when_its_body_raises(closed_scope):
    capi = closed_scope
    with pytest.raises(KeyError, match="from the body"):
        with capi.resident(max_references=3) as r:
            assert r.info()["active"] == 1
            raise KeyError("from the body")
    assert capi.ps_resident_info()["active"] == 0
    with capi.resident():                                              # and a scope can be opened again
        assert capi.ps_resident_info()["active"] == 1
        with pytest.raises(capi.PsError, match="open already"):
            with capi.resident():
                pass
        assert capi.ps_resident_info()["active"] == 1                  # the refused begin left the open scope alone
    assert capi.ps_resident_info()["active"] == 0
