"""Length of the dependent half-step chain of the persistent ensemble kernel, read off the gfx950 listing (no GPU needed).

A half step of the headline instantiation (d = 10, four point pairs per lane, 384 threads) is a relay: the hand-off wave
sees the two rows arrive, forms the proposal and reaches barrier A; the compute waves read the proposal, sum the kernel and
reach barrier B; the hand-off wave adds the wave partials, decides and stores the new row, which the next workgroup polls.
Everything between those points is latency of every one of the 4096 half steps of a benchmark step, so the listing is
held to three counts (`chain_counts`, in layout order, which is the order of the fast path):

  1. compute waves: the LDS round trips (batches of ds_read closed by an `s_waitcnt lgkmcnt`) between barrier A and the
     first fp64 arithmetic instruction -- the proposal and its in-bounds flag arrive together;
  2. hand-off wave: the instructions, and the branches and exec-mask instructions among them, between the
     `s_waitcnt vmcnt(0)` of the poll and barrier A;
  3. hand-off wave: the instructions between barrier B and the write-through store of the new row.

The same function on the listing of the commit before this file existed gave
  lgkm waits 2, round trips 2;  poll -> A 112 instructions, 30 of them control;  B -> store 56
(in that listing the stretch from the poll to barrier A also holds, in layout order, the blocks of the time-out and of the
exec-mask ladders around them; the fast path through it is about 70 instructions long).

The code object's metadata is held to one more thing: every instantiation of the kernel that the library contains -- the launch
table compiles exactly those that the fit rule (ens_stream_max_db) can select -- spills no register and uses no scratch memory.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alabi_amd", "csrc")
HEADLINE = "_ZN5alabi17ens_stream_kernelILi10ELi4ELi384ELb0EEEvNS_10StreamArgsE"

INSTRUCTION = re.compile(r"^\t([a-z][a-z0-9_]*)\b")
BARRIER = re.compile(r"^\ts_barrier\b")
FP64 = re.compile(r"^\tv_(fma|fmac|mul|add)_f64\b")
LGKM_WAIT = re.compile(r"^\ts_waitcnt\b.*\blgkmcnt\(")
VM_WAIT0 = re.compile(r"^\ts_waitcnt\b.*\bvmcnt\(0\)")
DS_READ = re.compile(r"^\tds_read_")
POLL = re.compile(r"^\tglobal_load_dwordx2\b.*\bsc1\b")
ROW_STORE = re.compile(r"^\tglobal_store_dwordx2\b.*\bsc1\b")
CONTROL = re.compile(r"^\t(s_cbranch_\w+|s_branch|s_and_saveexec_b64|s_or_saveexec_b64|s_andn2_saveexec_b64|"
                     r"s_(or|and|andn2|xor|mov)_b64\s+exec)\b")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def kernel_body(text, name):
    """The instruction lines of one kernel of a listing."""
    start = text.index("\n" + name + ":")
    end = text.index(".Lfunc_end", start)
    return [ln for ln in text[start:end].split("\n") if INSTRUCTION.match(ln)]


def chain_counts(body):
    """The three counts of the module docstring, from the instruction lines of the kernel."""
    barriers = [i for i, ln in enumerate(body) if BARRIER.match(ln)]
    # (1) the compute waves' loop is the stretch between two barriers that holds the kernel sum: the most fp64 arithmetic
    spans = list(zip(barriers, barriers[1:] + [len(body)]))
    a, b = max(spans, key=lambda s: sum(1 for ln in body[s[0]:s[1]] if FP64.match(ln)))
    first_fp64 = next(i for i in range(a, b) if FP64.match(body[i]))
    head = body[a + 1:first_fp64]
    waits = sum(1 for ln in head if LGKM_WAIT.match(ln))
    trips, open_reads = 0, False
    for ln in head:
        if DS_READ.match(ln):
            open_reads = True
        elif LGKM_WAIT.match(ln) and open_reads:
            trips, open_reads = trips + 1, False
    # (2) from the wait of the last poll load to the next barrier
    poll = max(i for i, ln in enumerate(body) if POLL.match(ln))
    wait = next(i for i in range(poll, len(body)) if VM_WAIT0.match(body[i]))
    bar_a = next(i for i in barriers if i > wait)
    to_a = body[wait + 1:bar_a]
    # (3) from the last barrier in front of the row store to the store
    store = next(i for i, ln in enumerate(body) if ROW_STORE.match(ln))
    bar_b = max(i for i in barriers if i < store)
    return {"lgkm_waits": waits, "lds_round_trips": trips,
            "poll_to_a": len(to_a), "poll_to_a_control": sum(1 for ln in to_a if CONTROL.match(ln)),
            "b_to_store": store - bar_b - 1}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("isa") / "ens_stream.s"
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--offload-device-only", "-S",
           os.path.join(CSRC, "ens_stream.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return out.read_text()


@pytest.fixture(scope="module")
def counts(listing):
    c = chain_counts(kernel_body(listing, HEADLINE))
    print(c)
    return c


def test_proposal_and_flag_arrive_in_one_lds_round_trip(counts):
    # every ds_read is issued before the first wait; the two waits are counted ones (the first read, then all)
    assert counts["lds_round_trips"] == 1
    assert counts["lgkm_waits"] <= 2


def test_poll_to_barrier_a_is_pinned(counts):
    # in layout order the stretch also holds the spin bookkeeping and the time-out block, 21 instructions that the fast
    # path branches over
    assert counts["poll_to_a"] == 53
    assert counts["poll_to_a_control"] == 7


def test_barrier_b_to_row_store_is_pinned(counts):
    assert counts["b_to_store"] == 22


def test_no_instantiation_spills(listing):
    kernels = {}
    for block in listing.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name and "ens_stream_kernel" in name.group(1):
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(
                r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    assert HEADLINE in kernels
    assert len(kernels) == 102      # the rows of the launch table: 55 squared-exponential, 47 generic
    for name, m in kernels.items():
        assert m == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (name, m)


if __name__ == "__main__":
    import sys
    print(chain_counts(kernel_body(open(sys.argv[1]).read(), HEADLINE)))
