"""CPU suite: the C-ABI library loads and exports every symbol include/glowtts_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(glowtts_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    so = os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(so)
    names = declared_symbols()
    assert len(names) >= 5
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/glowtts_hip.h but not exported"
    assert L.glowtts_abi_version() == 7


def test_product_path_has_no_oracle_import():
    """The product package must never import, dlopen or execute the oracle (or any CPU fallback of the GPU path): no mention of it in
    any Python or HIP / C++ source of the package, exactly one place that opens a shared library (`_lib.py`, the in-tree
    libglowtts_hip.so), no dlopen / system / popen in the native sources, no subprocess use in the package."""
    pkg = os.path.join(REPO, "glow_tts_amd")
    cdll_sites = []
    for root, _, files in os.walk(pkg):
        for f in files:
            path = os.path.join(root, f)
            if f.endswith(".py"):
                src = open(path).read()
                assert "oracle" not in re.sub(r"#.*", "", src).replace('"""', ""), f"{f} mentions oracle"
                assert not re.search(r"\bsubprocess\b|os\.system|os\.popen", src), f"{f} spawns processes"
                if re.search(r"ctypes\.(CDLL|cdll|PyDLL)|LoadLibrary", src):
                    cdll_sites.append(os.path.relpath(path, pkg))
            elif f.endswith((".hip", ".h", ".cpp", ".c")):
                src = open(path).read()
                assert "oracle" not in src.lower(), f"{f} mentions oracle"
                assert not re.search(r"\bdlopen\b|\bsystem\s*\(|\bpopen\b|\bexecv", src), f"{f} loads or executes external code"
    assert cdll_sites == ["_lib.py"], cdll_sites
    lib_src = open(os.path.join(pkg, "_lib.py")).read()
    assert 'LIB_PATH = os.path.join(_HERE, "libglowtts_hip.so")' in lib_src


def test_host_mas_twin_matches_core_pyx_vectors(golden_dir):
    """glowtts_mas_f32_host (the C-ABI twin of core.pyx:40 `maximum_path_c` for host-resident score matrices) on the golden
    vectors the reference's compiled core.pyx produced: paths and cumulative scores bit-exact; and the Python wrapper's signature."""
    import numpy as np
    import torch
    L = ctypes.CDLL(os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so"))
    from glow_tts_amd import abi
    _, L.glowtts_mas_f32_host.argtypes = abi.SIGNATURES["glowtts_mas_f32_host"]
    d = np.load(os.path.join(golden_dir, "mas_cases.npz"))
    for name in ["ragged", "ties", "square", "one_token", "x1000", "wide", "more_tokens"]:
        for threads in (1, 3):
            v = d[f"{name}/value"].copy()
            tx, ty = np.ascontiguousarray(d[f"{name}/t_x"], np.int32), np.ascontiguousarray(d[f"{name}/t_y"], np.int32)
            path = np.zeros(v.shape, np.int32)
            assert L.glowtts_mas_f32_host(v.ctypes.data, path.ctypes.data, tx.ctypes.data, ty.ctypes.data, *v.shape, -1e9, threads) == 0
            assert np.array_equal(path, d[f"{name}/path"].astype(np.int32)), name
            assert np.bitwise_xor.reduce(v.view(np.uint32).ravel()) == d[f"{name}/q_xor"], name
    from glow_tts_amd.monotonic_align import maximum_path_host
    v = torch.from_numpy(d["ragged/value"]).double()
    tx, ty = d["ragged/t_x"], d["ragged/t_y"]
    mask = torch.from_numpy(((np.arange(v.shape[1])[None, :, None] < tx[:, None, None]) & (np.arange(v.shape[2])[None, None, :] < ty[:, None, None])).astype(np.float64))
    p = maximum_path_host(v, mask)
    assert p.dtype == v.dtype and np.array_equal(p.numpy().astype(np.int32), d["ragged/path"].astype(np.int32))
    # more tokens than frames (no monotonic alignment): as core.pyx behaves - nothing accumulated, backtrack over the raw inputs (oracle C,
    # itself checked against the compiled core.pyx for such shapes, tests/golden/make_golden.py)
    from oracle import mas_ref
    rng = np.random.default_rng(3)
    w = rng.normal(-100, 30, (2, 40, 17)).astype(np.float32)
    txw, tyw = np.array([40, 31], np.int32), np.array([17, 9], np.int32)
    w *= ((np.arange(40)[None, :, None] < txw[:, None, None]) & (np.arange(17)[None, None, :] < tyw[:, None, None]))
    want, _ = mas_ref.maximum_path_c(w, txw, tyw, return_q=True)
    w2, pw = w.copy(), np.zeros(w.shape, np.int32)
    assert L.glowtts_mas_f32_host(w2.ctypes.data, pw.ctypes.data, txw.ctypes.data, tyw.ctypes.data, *w.shape, -1e9, 1) == 0
    assert np.array_equal(pw, want) and np.array_equal(w2, w)
    bad = np.array([v.shape[1] + 1] * v.shape[0], np.int32)
    vv = d["ragged/value"].copy(); pp = np.zeros(vv.shape, np.int32)
    assert L.glowtts_mas_f32_host(vv.ctypes.data, pp.ctypes.data, bad.ctypes.data, ty.ctypes.data, *vv.shape, -1e9, 1) == -1      # GLOWTTS_E_ARG


def test_model_deepcopy_and_state_dict_roundtrip_cpu():
    """The module stays an ordinary torch.nn.Module on the host: deepcopy (run-time caches dropped), state_dict round trip."""
    import copy, os, sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import tiny_hp_dict
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    m = GlowTTS(Recursive_Parse(tiny_hp_dict("Vanilla")))
    m._enc_cache["x"] = object()
    c = copy.deepcopy(m)
    assert c._enc_cache == {} and c._dec_stacks is None
    sd = m.state_dict()
    assert set(sd) == set(c.state_dict()) and all(torch.equal(sd[k], c.state_dict()[k]) for k in sd)
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(m.parameters(), c.parameters()))
    c.load_state_dict(sd, strict=True)


def test_collater_matches_reference_layout_and_buckets():
    """glow_tts_amd.data.Collater against a direct restatement of Datasets.py:23-39,67-74,225-250 (pad with '<E>', -Max_Abs_Mel, 0;
    truncate mels to a multiple of Num_Squeeze; mels transposed to [B, Mel, T]) and the bucketed / pinned variants."""
    import numpy as np
    import torch
    from glow_tts_amd.data import Collater
    rng = np.random.default_rng(0)
    batch = []
    for tt, tm in [(7, 41), (12, 33), (3, 58), (9, 2)]:
        batch.append((rng.integers(1, 40, tt), rng.standard_normal((tm, 5)).astype(np.float32), int(rng.integers(0, 9)),
                      rng.random(tm).astype(np.float32)))
    tok, tl, mel, ml, spk, ge2e, pit = Collater(num_squeeze=2, end_token_id=99, max_abs_mel=4.0)(batch)
    want_ml = [(len(m) // 2) * 2 for _, m, _, _ in batch]
    assert tl.tolist() == [7, 12, 3, 9] and ml.tolist() == want_ml and ge2e is None and spk.tolist() == [b[2] for b in batch]
    assert tok.shape == (4, 12) and mel.shape == (4, 5, max(want_ml)) and pit.shape == (4, max(want_ml))
    for b, (t, m, _, p) in enumerate(batch):
        assert tok[b, :len(t)].tolist() == t.tolist() and (tok[b, len(t):] == 99).all()
        assert torch.equal(mel[b, :, :want_ml[b]], torch.from_numpy(m[:want_ml[b]].T.copy())) and (mel[b, :, want_ml[b]:] == -4.0).all()
        n = min(len(p), pit.shape[1])
        assert torch.equal(pit[b, :n], torch.from_numpy(p[:n])) and (pit[b, n:] == 0).all()
    c2 = Collater(num_squeeze=2, end_token_id=99, token_buckets=[8, 16, 32], mel_buckets=[32, 64, 128], pin_memory=False)
    tok2, _, mel2, ml2, _, _, _ = c2(batch)
    assert tok2.shape == (4, 16) and mel2.shape == (4, 5, 64) and ml2.tolist() == want_ml
    assert torch.equal(tok2[:, :12], tok) and (tok2[:, 12:] == 99).all() and torch.equal(mel2[:, :, :max(want_ml)], mel)
    import pytest
    with pytest.raises(ValueError):
        Collater(token_buckets=[4])(batch)


def test_hot_kernels_use_no_scratch_memory(tmp_path):
    """Register-allocation guard: none of the kernels on the benchmarked path may spill (a DGATE epilogue variant once pushed the
    1024-thread LDS-DMA kernel from 90 to 128 VGPRs + 348 bytes of scratch and cost 2 % of the step).  Reads the code objects' metadata
    notes out of the built library (llvm-objdump --offloading + llvm-readelf --notes; nothing is executed)."""
    import re
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf")):
        pytest.skip("ROCm LLVM tools not found")
    so = os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so")
    shutil.copy(so, tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    objs = [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]
    assert objs, "no gfx950 code objects in the library"
    kernels = {}
    for f in objs:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for name, scratch, vgpr in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            kernels[name] = (int(scratch), int(vgpr))
    assert len(kernels) > 100
    hot = [r"wn_fwd_kernelILb1ELb0ELb1ELb0ELi0E", r"wn_bwd_kernel", r"conv_dma_kernelILi\dELi\dELi2ELb0E", r"conv_chain_kernel", r"conv_skinny_kernel", r"wgrad_kernel", r"attn_(fwd|bwd)_mfma_kernel",
           r"mas_dp_kernelILi[12]E", r"mas_dp2_kernel", r"ln_(fwd|bwd)_kernel", r"actnorm_inv", r"gate_bwd_kernel", r"mas_path_linear_kernel", r"expand_fwd4_kernel",
           r"squeeze_kernel", r"optim|radam|adam"]
    seen = {h: 0 for h in hot}
    for name, (scratch, vgpr) in kernels.items():
        for h in hot:
            if re.search(h, name):
                seen[h] += 1
                assert scratch == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
    for h, n in seen.items():
        assert n > 0 or h == r"optim|radam|adam", f"pattern {h} matched no kernel"


# ---------------------------------------------------------------------------------------------------------------------------------------
# glow_tts_amd/abi.py - the package's only restatement of include/glowtts_hip.h - against the header: signatures by parsing the prototypes,
# struct layouts through the C compiler, constants by value.  A wrong entry fails here, on the CPU, instead of truncating a pointer on the GPU.
# ---------------------------------------------------------------------------------------------------------------------------------------
HEADER = os.path.join(REPO, "include", "glowtts_hip.h")
C_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
STRUCT_RE = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)


def header_text():
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S))


def c_param_kind(decl):
    """`const float *x` -> "ptr", `int64_t rows` -> "int64_t"; an unknown type raises."""
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    kind = " ".join(words[:-1])                              # (every parameter of the header is named)
    if kind not in C_SCALARS:
        raise ValueError(f"parameter type of `{decl.strip()}` is not one the signature check knows")
    return kind


def header_prototypes(text):
    """name -> (return kind, [parameter kinds]) of every prototype.  Whatever is left of the header after the struct bodies, the preprocessor lines
    and the extern "C" braces must be a prototype of known return and parameter types: anything else raises instead of being skipped."""
    text = re.sub(r'extern\s+"C"\s*\{', " ", re.sub(r"(?m)^\s*#.*$", " ", STRUCT_RE.sub(" ", text)))
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"(\w+) (glowtts_\w+) ?\((.*)\)", stmt)
        if not m or m.group(1) not in ("int", "int64_t", "void") or m.group(2) in protos:
            raise ValueError(f"not a prototype the signature check knows: `{stmt}`")
        params = m.group(3).strip()
        protos[m.group(2)] = (m.group(1), [] if params == "void" else [c_param_kind(p) for p in params.split(",")])
    return protos


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return {v: k for k, v in C_SCALARS.items()}[t]           # (KeyError: a ctypes type no parameter of the header has)


def signature_errors(protos, table):
    errs = [f"{n}: in the header, not in abi.SIGNATURES" for n in protos.keys() - table.keys()]
    errs += [f"{n}: in abi.SIGNATURES, not in the header" for n in table.keys() - protos.keys()]
    for n in sorted(protos.keys() & table.keys()):
        (ret, params), (restype, argtypes) = protos[n], table[n]
        if ctypes_kind(restype) != ret:
            errs.append(f"{n}: returns {ret}, restype is {restype}")
        if len(params) != len(argtypes):
            errs.append(f"{n}: {len(params)} parameters, {len(argtypes)} argtypes")
            continue
        errs += [f"{n}: parameter {i} is {k}, argtypes[{i}] is {t}" for i, (k, t) in enumerate(zip(params, argtypes)) if ctypes_kind(t) != k]
    return errs


def header_structs(text):
    """C struct name -> field names in order (`int a, b;`, `const float *p, *q[N];` and array declarators handled)."""
    out = {}
    for tag, body, name in STRUCT_RE.findall(text):
        assert tag == name, (tag, name)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                fields += [re.fullmatch(r".*?(\w+)\s*(\[[^\]]*\])?\s*", d, re.S).group(1) for d in decl.split(",")]
        out[name] = fields
    return out


def c_layouts(structs, tmp_path):
    """C struct name -> (sizeof, [(field, offsetof, sizeof)]) as the system C compiler lays the header's structs out."""
    import subprocess
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    for s, fields in structs.items():
        lines.append(f'    printf("S {s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("F {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f in fields]
    lines += ['    return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([os.environ.get("CC", "cc"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = {}
    for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if w[0] == "S":
            out[w[1]] = (int(w[2]), [])
        else:
            out[w[1]][1].append((w[2], int(w[3]), int(w[4])))
    return out


def mirror_classes():
    from glow_tts_amd import abi
    return [v for v in vars(abi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure]


def layout_errors(layouts, mirrors):
    """Every header struct mirrored, every mirror's C struct present; per struct the same size, field count, names (a trailing underscore in Python
    ignored: `in_` is `in`) and (offset, size) sequence."""
    named = {}
    for m in mirrors:
        named.setdefault(getattr(m, "c_name", None), []).append(m)
    errs = [f"{s}: no mirror in abi.py" for s in layouts.keys() - named.keys()]
    for c_name, ms in named.items():
        for m in ms:
            if c_name not in layouts:
                errs.append(f"{m.__name__}: names `{c_name}`, which is no struct of the header")
                continue
            size, fields = layouts[c_name]
            mine = [(n.rstrip("_"), getattr(m, n).offset, getattr(m, n).size) for n, *_ in m._fields_]
            if ctypes.sizeof(m) != size:
                errs.append(f"{c_name}: sizeof is {size}, {m.__name__} has {ctypes.sizeof(m)}")
            if len(mine) != len(fields):
                errs.append(f"{c_name}: {len(fields)} fields, {m.__name__} has {len(mine)}")
            if [f[0] for f in mine] != [f[0] for f in fields]:
                errs.append(f"{c_name}: field names {[f[0] for f in fields]}, {m.__name__} has {[f[0] for f in mine]}")
            if [f[1:] for f in mine] != [f[1:] for f in fields]:
                errs.append(f"{c_name}: (offset, size) sequence {[f[1:] for f in fields]}, {m.__name__} has {[f[1:] for f in mine]}")
    return errs


def test_signature_table_matches_header_prototypes():
    from glow_tts_amd import abi
    protos = header_prototypes(header_text())
    assert set(protos) == set(declared_symbols())
    assert signature_errors(protos, abi.SIGNATURES) == []
    bench = {"glowtts_wavenet_fwd": (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),      # what bench.py assigns itself
             "glowtts_launch_count": (ctypes.c_int64, [ctypes.c_char_p]),
             "glowtts_mfma_clock_probe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p])}
    for n, sig in bench.items():
        assert abi.SIGNATURES[n] == sig, n
    with pytest.raises(ValueError):
        c_param_kind("double x")
    with pytest.raises(ValueError):
        header_prototypes("int glowtts_a(int n); typedef int glowtts_t;")


def test_struct_mirrors_match_compiled_layout(tmp_path):
    structs = header_structs(header_text())
    assert structs["glowtts_wn_bwd_job"] == ["dw", "v", "g", "inv_norm", "dv", "dg", "rows", "cols", "reserved"]
    assert structs["glowtts_flow_params"][3:7] == ["start", "in", "rs", "end"]
    assert layout_errors(c_layouts(structs, tmp_path), mirror_classes()) == []


def test_constants_match_header_defines():
    from glow_tts_amd import abi
    defines = {k: int(v) for k, v in re.findall(r"(?m)^\s*#define\s+GLOWTTS_(\w+)\s+(-?\d+)\s*$", header_text())}
    mine = {k: v for k, v in vars(abi).items() if k.isupper() and isinstance(v, int)}
    assert mine == defines                                   # every define restated, no constant of abi.py without one, equal values
    for p in ("PERM_", "APRO_", "EPI_", "F_", "WIO_", "IO_"):
        assert any(k.startswith(p) for k in defines), p
    for k in ("ABI_VERSION", "MAX_WN_LAYERS", "ROW_PAD", "WN_SLAB_BYTES", "PREP_MAX_JOBS", "SUM_MAX_SEGS", "WN_BWD_MAX_JOBS", "WN_FUSED_MAX_LAYERS"):
        assert k in defines


def test_abi_checks_report_a_wrong_signature_and_a_swapped_field(tmp_path):
    from glow_tts_amd import abi
    protos = header_prototypes(header_text())
    assert protos["glowtts_fill_zero"] == ("int", ["ptr", "int64_t", "ptr"])
    wrong = dict(abi.SIGNATURES, glowtts_fill_zero=(ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]))
    errs = signature_errors(protos, wrong)
    assert len(errs) == 1 and errs[0].startswith("glowtts_fill_zero: parameter 1 is int64_t")

    class Swapped(ctypes.Structure):                         # glowtts_wn_bwd_job with `int64_t rows` and `int cols` exchanged
        c_name = "glowtts_wn_bwd_job"
        _fields_ = [(n, ctypes.c_void_p) for n in ("dw", "v", "g", "inv_norm", "dv", "dg")] + [("cols", ctypes.c_int), ("rows", ctypes.c_int64), ("reserved", ctypes.c_int)]
    layouts = c_layouts(header_structs(header_text()), tmp_path)
    errs = layout_errors(layouts, [m for m in mirror_classes() if m.c_name != "glowtts_wn_bwd_job"] + [Swapped])
    assert errs and all(e.startswith("glowtts_wn_bwd_job:") for e in errs) and any("(offset, size)" in e for e in errs)


def test_package_declares_the_abi_in_one_place():
    pkg = os.path.join(REPO, "glow_tts_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and os.path.relpath(os.path.join(root, f), pkg) not in ("abi.py", "_lib.py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"\.argtypes|\.restype", src), f"{f} declares a signature: abi.SIGNATURES is the place"
                assert not re.search(r"\(\s*(ctypes\.)?(Structure|Union)\s*\)", src), f"{f} defines a ctypes structure: abi.py is the place"
    assert "CDLL" not in open(os.path.join(pkg, "abi.py")).read()


def test_loaded_library_is_bound_as_tabulated():
    from glow_tts_amd import _lib, abi
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _lib.lib()
    for n, (restype, argtypes) in abi.SIGNATURES.items():
        fn = getattr(L, n)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, n
    with pytest.raises(_lib.GlowTTSHipError, match="glowtts_not_there"):
        _lib._symbol(L, "glowtts_not_there")


# ---------------------------------------------------------------------------------------------------------------- the checked handle, _lib.api()
def test_value_returning_set_is_consistent_with_the_table():
    from glow_tts_amd import abi
    assert abi.VALUE_RETURNING <= set(abi.SIGNATURES)
    for n in abi.VALUE_RETURNING:
        assert abi.SIGNATURES[n][0] is ctypes.c_int, n
    assert {n for n in abi.SIGNATURES if "_supported" in n} <= abi.VALUE_RETURNING
    assert {"glowtts_abi_version", "glowtts_opt_chunk"} <= abi.VALUE_RETURNING


def test_checked_handle_is_bound_as_tabulated_and_checks_exactly_the_statuses():
    from glow_tts_amd import _lib, abi
    L, A = _lib.lib(), _lib.api()
    assert A is _lib.api() and L is _lib.lib()
    assert set(vars(A)) == set(abi.SIGNATURES)
    for n, (restype, argtypes) in abi.SIGNATURES.items():
        raw, fn = getattr(L, n), getattr(A, n)
        assert fn is not raw, n
        assert fn.restype is restype and list(fn.argtypes) == argtypes, n
        assert (fn.errcheck is not None) == (restype is ctypes.c_int and n not in abi.VALUE_RETURNING), n
        assert raw.errcheck is None, n


def test_checked_handle_raises_on_a_status_and_passes_values_through():
    from glow_tts_amd import _lib, abi
    row = (None,) * 9 + (1, 4, 256, 64, 64, 80, 1, 0, None)                  # every pointer NULL: refused before anything is launched (no device is touched)
    with pytest.raises(_lib.GlowTTSHipError, match=r"glowtts_pwg_layer_bf16 failed with code -1"):
        _lib.api().glowtts_pwg_layer_bf16(*row)
    assert _lib.lib().glowtts_pwg_layer_bf16(*row) == abi.E_ARG
    assert _lib.api().glowtts_pwg_supported(64, 128, 64, 80, 1) == 1
    assert _lib.api().glowtts_pwg_supported(60, 120, 64, 80, 1) == 0


def test_no_call_site_checks_a_status_by_hand():
    for top in ("glow_tts_amd", "tools"):
        for root, _, files in os.walk(os.path.join(REPO, top)):
            for f in files:
                path = os.path.join(root, f)
                if f.endswith(".py") and os.path.relpath(path, REPO) != os.path.join("glow_tts_amd", "_lib.py"):
                    assert "_lib.check(" not in open(path).read(), f"{os.path.relpath(path, REPO)} checks a status by hand: call through _lib.api()"
