"""The Cholesky task lists, pinned: sha256 digests of what the three host-only debug hooks return over a grid that touches every
list-shaping switch, compared with tests/golden/chol_task_lists.json.  The digests were recorded from the library of the commit
before the lists and the environment switches moved into chol_tasklist.hip (`python tests/test_chol_task_lists_pinned.py LIB`
prints them for any libalabi_hip.so), so a change of any list, default or accepted switch value shows here.  No GPU needed."""
import ctypes
import hashlib
import itertools
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chol_task_lists.json")
SWITCHES = ["ALABI_CHOL_GK", "ALABI_CHOL_NEAR", "ALABI_CHOL_W8", "ALABI_CHOL_UPDATE2", "ALABI_CHOL_UPDATE4",
            "ALABI_BATCH_GK", "ALABI_BATCH_LEFT", "ALABI_BATCH_PHASES"]
BATCHES = [[25] * 6 + [16] * 5 + [40] * 2, [3, 5, 16, 33, 40, 25, 25, 7, 12], [40, 16, 25, 25, 16, 40, 31, 31, 8, 8, 8, 20, 20, 20, 20, 20, 20]]


def _grid():
    """(case id, hook, arguments, environment) of every pinned list"""
    single = [{}] + [{"ALABI_CHOL_GK": g, "ALABI_CHOL_NEAR": n} for g, n in (("1", "1"), ("4", "2"), ("8", "3"))]
    single += [{"ALABI_CHOL_W8": "0"}, {"ALABI_CHOL_W8": "1"}, {"ALABI_CHOL_UPDATE2": "0"}, {"ALABI_CHOL_UPDATE4": "0"}, {"ALABI_CHOL_UPDATE4": "1"}]
    for nb, env in itertools.product((3, 5, 16, 33, 40, 79, 100, 157, 256), single):
        yield "single", (nb,), env
    for nb, gk, left, u4 in itertools.product((16, 25, 40), ("4", "10", "32"), ("0", "1"), (None, "0")):
        env = {"ALABI_BATCH_GK": gk, "ALABI_BATCH_LEFT": left}
        if u4 is not None:
            env["ALABI_CHOL_UPDATE4"] = u4
        yield "batch_matrix", (nb,), env
    for b, (nlists, window), phases in itertools.product(range(len(BATCHES)), ((8, 8), (4, 0), (1, 3)), (None, "0", "3")):
        yield "batch", (b, nlists, window), ({} if phases is None else {"ALABI_BATCH_PHASES": phases})


def _case_id(hook, args, env):
    return " ".join([hook, ",".join(map(str, args))] + ["%s=%s" % kv for kv in sorted(env.items())])


CASES = {_case_id(*c): c for c in _grid()}


def _load(path):
    lib = ctypes.CDLL(path)
    ip = ctypes.POINTER(ctypes.c_int)
    lib.alabi_debug_chol_tasks.argtypes = [ctypes.c_int, ip, ctypes.c_int]
    lib.alabi_debug_chol_batch_matrix_tasks.argtypes = [ctypes.c_int, ip, ctypes.c_int]
    lib.alabi_debug_chol_batch_tasks.argtypes = [ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ip]
    return lib


def _digest(lib, hook, args, env):
    """sha256 over the list's (type, i, j, k) quadruples as native ints (the batch: followed by its list offsets); the
    environment holds exactly `env` of the list-shaping switches while the hook runs"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        if hook == "batch":
            b, nlists, window = args
            nbs = (ctypes.c_int * len(BATCHES[b]))(*BATCHES[b])
            n = lib.alabi_debug_chol_batch_tasks(len(nbs), nbs, nlists, window, None, 0, None)
            buf, lo = (ctypes.c_int * (4 * n))(), (ctypes.c_int * (nlists + 1))()
            assert lib.alabi_debug_chol_batch_tasks(len(nbs), nbs, nlists, window, buf, n, lo) == n
            return hashlib.sha256(bytes(buf) + bytes(lo)).hexdigest()
        fn = lib.alabi_debug_chol_tasks if hook == "single" else lib.alabi_debug_chol_batch_matrix_tasks
        n = fn(args[0], None, 0)
        buf = (ctypes.c_int * (4 * n))()
        assert fn(args[0], buf, n) == n
        return hashlib.sha256(bytes(buf)).hexdigest()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def lib():
    from alabi_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _load(_lib.LIB_PATH)


def test_golden_file_covers_the_grid_exactly():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_task_list_matches_its_pinned_digest(lib, case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    assert _digest(lib, *CASES[case]) == want


if __name__ == "__main__":
    json.dump({c: _digest(_load(sys.argv[1]), *CASES[c]) for c in sorted(CASES)}, sys.stdout, indent=0, sort_keys=True)
    print()
