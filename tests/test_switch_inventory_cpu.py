"""CPU: the environment switches of the native library are read in one place and listed in one place.

(a) No file of csrc/ but env.h touches the environment.  (b) The names the sources pass to the env_* helpers of env.h are exactly
the names of the switch table in DESIGN.md section 9.1, and each name is read at one place in the source: a switch that is added,
renamed or removed without its row (or a row without its switch) fails here, as does a second read of one switch."""
import re
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "music2midi_amd" / "csrc"
SOURCES = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h"))
HELPER_CALL = re.compile(r'\benv_(?:on|set|int|str)\(\s*"(M2M_[A-Z0-9_]+)"')
HELPER_ANY = re.compile(r"\benv_(?:on|set|int|str)\(\s*([^)\s,]+)")


def _code(path):
    """the file without // comments (the sources have no block comments that mention the environment)"""
    return "\n".join(line.split("//", 1)[0] for line in path.read_text().splitlines())


def test_only_env_h_touches_the_environment():
    assert (CSRC / "env.h").exists()
    for src in SOURCES:
        if src.name == "env.h":
            continue
        assert "getenv" not in src.read_text(), f"{src.name} mentions getenv: the environment is read through csrc/env.h only"
        assert not re.search(r"\b(environ|putenv|setenv)\b", _code(src)), f"{src.name} touches the environment"


def _names_in_source():
    names = Counter()
    for src in SOURCES:
        code = _code(src)
        if src.name != "env.h":
            # every helper call names its switch as a literal, so that the extraction below sees it
            for arg in HELPER_ANY.findall(code):
                assert arg.startswith('"M2M_'), f"{src.name}: env helper called with {arg}, not with a \"M2M_...\" literal"
        names.update(HELPER_CALL.findall(code))
    return names


def _names_in_design():
    text = (ROOT / "DESIGN.md").read_text()
    start = text.index("### 9.1 Switches of the native library")
    end = text.index("\n## ", start)
    names = []
    for line in text[start:end].splitlines():
        if not line.startswith("| `M2M_"):
            continue
        first = line.split("|")[1]
        names += re.findall(r"`(M2M_[A-Z0-9_]+)`", first)
    return names


def test_switch_table_matches_the_source():
    src = _names_in_source()
    doc = _names_in_design()
    assert len(src) >= 50, sorted(src)                      # the extraction itself works
    assert len(doc) == len(set(doc)), [n for n, c in Counter(doc).items() if c > 1]
    assert set(doc) == set(src), {"only in DESIGN.md": sorted(set(doc) - set(src)), "only in csrc": sorted(set(src) - set(doc))}
    assert "M2M_CHAIN_CU_MASK" not in src and "M2M_CHAIN_CU_MASK_MODE" not in src


def test_every_switch_is_read_at_one_place():
    twice = {n: c for n, c in _names_in_source().items() if c > 1}
    assert not twice, twice
