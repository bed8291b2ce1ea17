#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel: the proof a host-only refactor needs that no kernel moved.

    python tools/kernel_text_diff.py PARENT_CSRC [NEW_CSRC]        (NEW_CSRC: this tree's music2midi_amd/csrc)

Every *.hip of both directories is compiled to gfx950 assembly with the product's flags (-S --cuda-device-only).  The text of
every function (its label up to its .Lfunc_end, the kernel descriptor included) is compared by symbol over the UNION of each
tree's files, so a kernel may move between files; a file present in both trees with the same name is also compared whole.
Masked: the per-file __hip_cuid_ symbol, and the ordinal of the function within its file that local labels carry
(.LBB<n>_ and BB<n>_ in the loop comments, .Lfunc_end<n>; the padding in front of a comment follows the label's width), which
changes for every function behind one that moved out of the file.
"""
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from music2midi_amd.csrc.build import FLAGS, _hipcc  # noqa: E402


def assembly(src: Path, out: Path) -> str:
    r = subprocess.run([_hipcc(), *FLAGS, "-S", "--cuda-device-only", str(src), "-o", str(out)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", out.read_text())


def functions(text: str) -> dict:
    out, name, body = {}, None, []
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s+; @", line)
        if m and name is None:
            name, body = m.group(1), []
        if name is not None:
            body.append(re.sub(r"\s+;", " ;", re.sub(r"(LBB|BB|Lfunc_end|Lfunc_begin)\d+", r"\1", line)))
            if line.startswith(".Lfunc_end"):
                assert name not in out, name
                out[name] = "\n".join(body)
                name = None
    return out


def tree(csrc: Path, tmp: Path) -> dict:
    srcs = sorted(csrc.glob("*.hip"))
    tmp.mkdir()
    with ThreadPoolExecutor(max_workers=8) as ex:
        texts = list(ex.map(lambda s: assembly(s, tmp / (s.stem + ".s")), srcs))
    return {s.name: t for s, t in zip(srcs, texts)}


def main() -> int:
    parent = Path(sys.argv[1])
    new = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).resolve().parents[1] / "music2midi_amd" / "csrc"
    with tempfile.TemporaryDirectory() as td:
        a, b = tree(parent, Path(td) / "a"), tree(new, Path(td) / "b")
    bad = 0
    whole = [n for n in a if n in b and a[n] == b[n]]
    print(f"files identical as a whole: {len(whole)} of {len(a)} ({', '.join(whole)})")
    changed = [n for n in set(a) | set(b) if n not in whole]
    fa, fb = {}, {}
    for side, dst in ((a, fa), (b, fb)):
        for n in changed:
            for sym, body in functions(side.get(n, "")).items():
                assert sym not in dst, f"{sym} defined twice"
                dst[sym] = (n, body)
    for sym in sorted(set(fa) | set(fb)):
        if sym not in fa or sym not in fb:
            print(f"ONLY IN {'parent' if sym in fa else 'new'}: {sym}")
            bad += 1
        elif fa[sym][1] != fb[sym][1]:
            print(f"DIFFERS: {sym} ({fa[sym][0]} -> {fb[sym][0]})")
            bad += 1
    moved = sum(1 for s in fa if s in fb and fa[s][0] != fb[s][0])
    print(f"files that differ: {sorted(changed)}; functions compared: {len(fa)} parent / {len(fb)} new, {moved} moved to another file, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
