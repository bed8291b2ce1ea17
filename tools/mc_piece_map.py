#!/usr/bin/env python3
"""Which instantiations of dec_attn_mc_kernel change text when ONE shared per-row piece replaces its hand-written copy.

    git show <parent>:music2midi_amd/csrc/decode.hip > /tmp/parent_decode.hip
    python tools/mc_piece_map.py /tmp/parent_decode.hip [piece ...]          (default: every tools/mc_pieces/*.patch, then all together)

Each tools/mc_pieces/<piece>.patch puts one piece into the parent's kernel (the parent: the commit before dec_attn_mc_kernel called
any of them).  The patched copy is compiled to gfx950 assembly with the product's flags next to the parent's file, and the
functions are compared as tools/kernel_text_diff.py compares them.  Per piece: how many functions differ, how many of them are not
dec_attn_mc_kernel (must be 0 unless the piece itself changed), WORSE lines (more scratch, more LDS, less occupancy), and the
resources parent -> new of every instantiation that moved.  Nothing runs on a device.
"""
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import kernel_text_diff as ktd  # noqa: E402

PIECES = Path(__file__).resolve().parent / "mc_pieces"
NEEDS = {"f_merge": ["e_softmax"]}          # da_merge takes the DaSoftmax: its patch applies on top of e_softmax's
CSRC = Path(__file__).resolve().parents[1] / "music2midi_amd" / "csrc"


def assembly(src: Path) -> str:
    return ktd.assembly(src, src.with_suffix(".s"))


def patched(parent: Path, names, out: Path) -> Path:
    out.write_text(parent.read_text())
    for n in names:
        subprocess.run(["patch", "-s", "--no-backup-if-mismatch", str(out), str(PIECES / f"{n}.patch")], check=True)
    return out


def main() -> int:
    parent = Path(sys.argv[1])
    every = sorted(p.stem for p in PIECES.glob("*.patch"))
    cases = [NEEDS.get(n, []) + [n] for n in (sys.argv[2:] or every)] + ([] if sys.argv[2:] else [every])
    ktd.FLAGS.append(f"-I{CSRC}")      # the copies' headers: this tree's
    with tempfile.TemporaryDirectory() as td:
        srcs = [patched(parent, [], Path(td) / "parent.hip")] + [patched(parent, c, Path(td) / ("_".join(c) + ".hip")) for c in cases]
        with ThreadPoolExecutor(max_workers=8) as ex:
            texts = list(ex.map(assembly, srcs))
    pinfo = {}
    pf = ktd.functions(texts[0], pinfo)
    for case, text in zip(cases, texts[1:]):
        info = {}
        f = ktd.functions(text, info)
        differ = [s for s in sorted(set(pf) & set(f)) if pf[s] != f[s]]
        names = ktd.demangled(differ)
        lines, worse = [], 0
        for s in differ:
            p, n = pinfo.get(s, {}), info.get(s, {})
            w = n.get("scratch", 0) > p.get("scratch", 0) or n.get("lds", 0) > p.get("lds", 0) or n.get("occ", 0) < p.get("occ", 0)
            worse += w
            lines.append(f"    {names[s]}: " + ", ".join(f"{c} {p.get(c, '?')} -> {n.get(c, '?')}" for c in ktd.COLUMNS) + ("  WORSE" if w else ""))
        other = sum("dec_attn_mc_kernel" not in names[s] for s in differ)
        print(f"{' + '.join(case)}: {len(pf)} parent / {len(f)} new functions, {len(set(pf) ^ set(f))} on one side only, {len(differ)} differ, "
              f"{other} of them not dec_attn_mc_kernel, {worse} WORSE")
        print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
