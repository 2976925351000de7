"""The verdict looks of the pair kernel's hand-off wave, read off the gfx950 listing (no GPU needed).

Between barrier A and barrier B of a class-1 item the hand-off wave of ens_pair_kernel polls the verdict of the fresh input row.
Two other forms of that poll were built and measured -- a first look delayed by a compile-time `s_sleep`, and a ring of two or
three looks in flight -- after the look counters (alabi_ens_pair_stats3) had shown that four of five polls are decided by their
FIRST look; both were slower and neither is kept (NOTES.md, "Pair kernel: the verdict looks, counted").  The listing is held to
the form that stays, for the headline instantiation (squared exponential, d = 10, four point pairs per lane) and for one of the
generic family:

  * the kernel has no `s_sleep`: nothing delays a look;
  * exactly one place issues three write-through loads back to back -- the verdict look: the verdict word and the two
    fetched-ahead words of the next item -- and the first wait behind it is `s_waitcnt vmcnt(2)`: the loop waits for the
    verdict word alone, the fetched-ahead words are waited for behind the loop;
  * every other write-through look has two loads (the input poll's reload, the fetch-ahead of an item without a verdict poll).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alabi_amd", "csrc")

INSTRUCTION = re.compile(r"^\t([a-z][a-z0-9_]*)\b")
SLEEP = re.compile(r"^\ts_sleep\s+(\d+)")
POLL = re.compile(r"^\tglobal_load_dwordx2\b.*\bsc1\b")
VM_WAIT = re.compile(r"^\ts_waitcnt\b.*\bvmcnt\((\d+)\)")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _pair_kernel(d, ppt, tmax, generic):
    return "_ZN5alabi15ens_pair_kernelILi%dELi%dELi%dELb%dEEEvNS_8PairArgsE" % (d, ppt, tmax, int(generic))


def kernel_body(text, name):
    """The instruction lines of one kernel of a listing."""
    start = text.index("\n" + name + ":")
    end = text.index(".Lfunc_end", start)
    return [ln for ln in text[start:end].split("\n") if INSTRUCTION.match(ln)]


def look_groups(body):
    """(number of write-through loads issued back to back, vmcnt of the first wait behind them) for every such run."""
    groups, i = [], 0
    while i < len(body):
        if not POLL.match(body[i]):
            i += 1
            continue
        n = 0
        while POLL.match(body[i + n]):
            n += 1
        wait = next((int(VM_WAIT.match(ln).group(1)) for ln in body[i + n:] if VM_WAIT.match(ln)), None)
        groups.append((n, wait))
        i += n
    return groups


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("isa") / "ens_pair.s"
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--offload-device-only", "-S",
           os.path.join(CSRC, "ens_pair.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return out.read_text()


# the headline instantiation (C3), and the generic family at five dimensions
@pytest.mark.parametrize("d,ppt,generic", [(10, 4, False), (5, 1, True)])
def test_verdict_look_is_three_loads_and_waits_for_the_verdict_alone(listing, d, ppt, generic):
    body = kernel_body(listing, _pair_kernel(d, ppt, 384, generic))
    groups = look_groups(body)
    print(groups)
    assert not any(SLEEP.match(ln) for ln in body)
    assert [g for g in groups if g[0] == 3] == [(3, 2)]
    assert all(g[0] in (2, 3) for g in groups), groups


if __name__ == "__main__":
    import sys
    print(look_groups(kernel_body(open(sys.argv[1]).read(), _pair_kernel(10, 4, 384, False))))
