"""plan.py re-declares the step-table layout and the constants of include/vbn_hip_types.h and
csrc/*.h; this compares the two sides from the header text (no compiler, no GPU)."""
import os
import re

from vectorizedbayesiannetwork_amd import plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorizedbayesiannetwork_amd", "csrc")


def _read(path):
    with open(path) as f:
        return f.read()


TYPES = _read(os.path.join(ROOT, "include", "vbn_hip_types.h"))
WALK = "\n".join(_read(os.path.join(CSRC, n)) for n in sorted(os.listdir(CSRC)) if n.endswith(".h"))


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _header_values(text):
    """name -> int of every ``#define NAME <int>`` and every ``NAME = <int>`` enumerator."""
    text = _strip_comments(text)
    out = {}
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\d+)[uU]?[ \t]*(?://.*)?$", text, flags=re.M):
        assert name not in out, name
        out[name] = int(val)
    for body in re.findall(r"\benum\s+\w+\s*\{(.*?)\}", text, flags=re.S):
        for name, val in re.findall(r"(\w+)\s*=\s*(\d+)", body):
            assert name not in out, name
            out[name] = int(val)
    return out


def test_step_field_order():
    """vbn_step's 32 fields, in order, are plan.py's S_* indices (aliases share their base word)."""
    body = re.search(r"typedef struct vbn_step \{(.*?)\} vbn_step;", TYPES, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"int32_t([^;]*);", _strip_comments(body)) for f in decl.split(",")]
    s_name = {"n_in": "S_NIN", "in_off": "S_INOFF", "out_col": "S_OUTCOL", "out_dim": "S_OUTDIM",
              "fixed_col": "S_FIXEDCOL", "n_out": "S_NOUT", "node_id": "S_NODEID", "noise_idx": "S_NOISE"}
    assert len(fields) == len(set(fields)) == P.STEP_INTS == 32
    for word, f in enumerate(fields):
        assert getattr(P, s_name.get(f, "S_" + f.upper())) == word, f
    s_all = {k: v for k, v in vars(P).items() if re.fullmatch(r"S_[A-Z0-9_]+", k)}
    aliases = {"S_ZLIM": "off_kq", "S_OFF_W3H": "off_kqy", "S_OFF_KMT2": "off_w1"}
    assert len(s_all) == 32 + len(aliases)
    assert sorted(v for k, v in s_all.items() if k not in aliases) == list(range(32))
    for k, base in aliases.items():
        assert s_all[k] == fields.index(base), k


def test_enums_and_flags_match_both_ways():
    hv = _header_values(TYPES)
    single = {"ROLE": "ROLE_", "F": "F_", "MODE": "MODE_", "KM": "KM_"}      # VBN_X_NAME <-> plan.X_NAME
    tables = {"KIND": P.KIND_ID, "ACT": P.ACT_ID, "WITHIN": P.WITHIN_ID}     # VBN_X_NAME <-> plan.X_ID["name"]
    header, host = {}, {}
    for name, val in hv.items():
        m = re.fullmatch(r"VBN_(KIND|ROLE|F|ACT|WITHIN|MODE|KM)_(\w+)", name)
        if m:
            header[(m.group(1), m.group(2))] = val
    for group, prefix in single.items():
        for k, v in vars(P).items():
            if k.startswith(prefix) and isinstance(v, int):
                host[(group, k[len(prefix):])] = v
    for group, table in tables.items():
        for k, v in table.items():
            host[(group, k.upper())] = v
    assert header == host, sorted(set(header.items()) ^ set(host.items()))
    assert {g for g, _ in header} == set(single) | set(tables)


def test_shared_kde_and_staging_constants():
    hv = _header_values(WALK)
    for h_name, p_name in (("KDE_CHUNKS", "KDE_CHUNKS"), ("KDE_REC_TAIL", "KDE_REC_TAIL"),
                           ("KDE_HALF_MIN", "KDE_HALF_MIN"), ("KDE_MT_HEAD", "KDE_MT_HEADER"),
                           ("KDE_MT_GROUP", "KDE_MT_GROUP"), ("KDE_MT2_HEAD", "KDE_MT2_HEADER"),
                           ("KDE_MT2_K", "KDE_MT2_K"), ("WBLK_CHUNK", "WBLK_CHUNK")):
        assert hv[h_name] == getattr(P, p_name), h_name
    assert hv["KDE_MT2_ROW4"] * 4 == P.KDE_MT2_ROW
    assert P.STEP_INTS * 4 == 128
    assert re.search(r"sizeof\(vbn_step\) == 128", TYPES)
