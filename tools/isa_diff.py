#!/usr/bin/env python3
"""Compare the device code of two builds symbol by symbol:  isa_diff.py OLD NEW

OLD and NEW are outputs of `hipcc <the Makefile's flags> --offload-device-only -S file.hip -o file.s`, or folders of them.
Every function (label .. .Lfunc_end) is reduced to its instructions -- comments and directives dropped, local labels
renumbered in order of appearance -- and reported as same / DIFF / MISSING / EXTRA, then the per-kernel metadata is compared.
Exit status 1 on any difference.  A refactor that only moves device code must come out without one.
"""
import pathlib, re, sys

META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")

def load(path):
    p = pathlib.Path(path)
    text = "\n".join(f.read_text() for f in (sorted(p.glob("*.s")) if p.is_dir() else [p]))
    funcs, kerns, name, cur, local = {}, [], None, None, {}
    for raw in text.split("\n"):
        line = raw.split(";")[0].strip()
        if raw.startswith("  - ."): kerns.append({})                  # an entry of amdhsa.kernels opens
        m = re.match(r"(?:- )?\.(\w+):\s+(\S+)$", line)
        if m and kerns and m.group(1) in META + ("symbol",): kerns[-1][m.group(1)] = m.group(2)
        if line.startswith(".Lfunc_end"):                                  # only what .Lfunc_end closes is a function
            if cur is not None: funcs[name] = cur
            cur = None
        elif re.match(r"[A-Za-z_][\w$.]*:$", line): name, cur, local = line[:-1], [], {}
        elif cur is not None and line and (line.startswith(".L") or not line.startswith(".")):
            cur.append(re.sub(r"\.L(BB|tmp|func_\w+?)\d+(_\d+)?", lambda t: local.setdefault(t.group(0), ".L%d" % len(local)), line))
    return funcs, {k.pop("symbol"): k for k in kerns if "symbol" in k}

def main(old, new):
    (fo, mo), (fn, mn) = load(old), load(new)
    bad = 0
    for name in sorted(set(fo) | set(fn)):
        state = "MISSING" if name not in fn else "EXTRA" if name not in fo else "same" if fo[name] == fn[name] else "DIFF"
        bad += state != "same"
        print("%-8s %s (%s instructions)" % (state, name, len(fn.get(name, fo.get(name)))))
    for name in sorted(set(mo) | set(mn)):
        if mo.get(name) != mn.get(name):
            bad += 1
            print("METADATA %s: %s -> %s" % (name, mo.get(name), mn.get(name)))
    print("%d symbols, %d kernels with metadata, %d differences" % (len(set(fo) | set(fn)), len(set(mo) | set(mn)), bad))
    return 1 if bad else 0

if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
