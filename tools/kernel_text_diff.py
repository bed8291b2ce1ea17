#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel: the proof a host-only refactor needs that no kernel moved.

    python tools/kernel_text_diff.py [--resources] PARENT_CSRC [NEW_CSRC]        (NEW_CSRC: this tree's music2midi_amd/csrc)

Every *.hip of both directories is compiled to gfx950 assembly with the product's flags (-S --cuda-device-only).  The text of
every function (its label up to its .Lfunc_end, the kernel descriptor included) is compared by symbol over the UNION of each
tree's files, so a kernel may move between files; a file present in both trees with the same name is also compared whole.
Masked: the per-file __hip_cuid_ symbol, and the ordinal of the function within its file that local labels carry
(.LBB<n>_ and BB<n>_ in the loop comments, .Lfunc_end<n>; the padding in front of a comment follows the label's width), which
changes for every function behind one that moved out of the file.

--resources: for a device-code refactor, where text may move but allocations may not.  Every function that differs is followed
by parent -> new of code bytes, VGPRs, AGPRs, SGPRs, scratch, static LDS and occupancy, read from the "Kernel info" comment block the
compiler writes behind each function (no instruction text is looked at); a line ends in "WORSE" where scratch or LDS went up or
occupancy went down, and their count is printed last.
"""
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from music2midi_amd.csrc.build import FLAGS, _hipcc  # noqa: E402

# label in the "Kernel info" block -> column of the report
INFO = {"codeLenInByte": "code", "NumVgprs": "vgpr", "NumAgprs": "agpr", "TotalNumSgprs": "sgpr", "NumSgprs": "sgpr",
        "ScratchSize": "scratch", "LDSByteSize": "lds", "Occupancy": "occ"}
COLUMNS = ("code", "vgpr", "agpr", "sgpr", "scratch", "lds", "occ")


def assembly(src: Path, out: Path) -> str:
    r = subprocess.run([_hipcc(), *FLAGS, "-S", "--cuda-device-only", str(src), "-o", str(out)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", out.read_text())


def functions(text: str, info: dict = None) -> dict:
    """symbol -> text; `info`, if given, receives symbol -> {column: value} from the comment block behind the function"""
    out, name, body, last = {}, None, [], None
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s+; @", line)
        if m and name is None:
            name, body = m.group(1), []
        if name is not None:
            body.append(re.sub(r"\s+;", " ;", re.sub(r"(LBB|BB|Lfunc_end|Lfunc_begin)\d+", r"\1", line)))
            if line.startswith(".Lfunc_end"):
                assert name not in out, name
                out[name] = "\n".join(body)
                name, last = None, name
        elif info is not None and last is not None:
            m = re.match(r"^; (\w+)\s*[:=]\s*(\d+)", line)
            if m and m.group(1) in INFO:
                info.setdefault(last, {}).setdefault(INFO[m.group(1)], int(m.group(2)))
    return out


def tree(csrc: Path, tmp: Path) -> dict:
    srcs = sorted(csrc.glob("*.hip"))
    tmp.mkdir()
    with ThreadPoolExecutor(max_workers=8) as ex:
        texts = list(ex.map(lambda s: assembly(s, tmp / (s.stem + ".s")), srcs))
    return {s.name: t for s, t in zip(srcs, texts)}


def demangled(symbols) -> dict:
    try:
        r = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True)
        return dict(zip(symbols, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}


def main() -> int:
    args = [x for x in sys.argv[1:] if x != "--resources"]
    resources = len(args) != len(sys.argv) - 1
    parent = Path(args[0])
    new = Path(args[1]) if len(args) > 1 else Path(__file__).resolve().parents[1] / "music2midi_amd" / "csrc"
    with tempfile.TemporaryDirectory() as td:
        a, b = tree(parent, Path(td) / "a"), tree(new, Path(td) / "b")
    bad = 0
    whole = [n for n in a if n in b and a[n] == b[n]]
    print(f"files identical as a whole: {len(whole)} of {len(a)} ({', '.join(whole)})")
    changed = [n for n in set(a) | set(b) if n not in whole]
    fa, fb, ia, ib = {}, {}, {}, {}
    for side, dst, info in ((a, fa, ia), (b, fb, ib)):
        for n in changed:
            for sym, body in functions(side.get(n, ""), info).items():
                assert sym not in dst, f"{sym} defined twice"
                dst[sym] = (n, body)
    differ = []
    for sym in sorted(set(fa) | set(fb)):
        if sym not in fa or sym not in fb:
            print(f"ONLY IN {'parent' if sym in fa else 'new'}: {sym}")
            bad += 1
        elif fa[sym][1] != fb[sym][1]:
            differ.append(sym)
            bad += 1
    names = demangled(differ) if resources else {}
    worse = 0
    for sym in differ:
        print(f"DIFFERS: {sym} ({fa[sym][0]} -> {fb[sym][0]})")
        if resources:
            p, n = ia.get(sym, {}), ib.get(sym, {})
            is_worse = n.get("scratch", 0) > p.get("scratch", 0) or n.get("lds", 0) > p.get("lds", 0) or n.get("occ", 0) < p.get("occ", 0)
            worse += is_worse
            cols = ", ".join(f"{c} {p.get(c, '?')} -> {n.get(c, '?')}" for c in COLUMNS)
            print(f"    {names[sym]}\n    {cols}{'  WORSE' if is_worse else ''}")
    moved = sum(1 for s in fa if s in fb and fa[s][0] != fb[s][0])
    print(f"files that differ: {sorted(changed)}; functions compared: {len(fa)} parent / {len(fb)} new, {moved} moved to another file, {bad} mismatches")
    if resources:
        print(f"differing functions with more scratch, more LDS or less occupancy than the parent's: {worse}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
