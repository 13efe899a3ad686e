"""CPU checks of the drop-in boundary: the C-ABI library builds, loads and exports every
entry point include/f16env.h declares; the Python mirror matches the header; the product
package never reaches into oracle/ (no CPU fallback)."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "f16env.h")


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def declared_functions():
    return sorted(set(re.findall(r"\b(f16env_\w+)\s*\(", header_source())))


# ---- the header, parsed: what the binding (_lib.SIGNATURES, abi.STRUCTS, abi's constants) is held against
def parse_header(src=None):
    """{"functions": {name: (return type, [parameter type, ...])} in the header's order,
    "struct_fields": {struct: number of fields its body declares}, "constants": {name: value} of
    every numeric #define F16* and every enumerator}. Types are spelled without const and spaces."""
    src = header_source() if src is None else src
    spell = lambda t: re.sub(r"\bconst\b|\s+", "", t)  # noqa: E731
    functions = {}
    for ret, name, params in re.findall(r"^([\w ]+?\**)\s*\b(f16env_\w+)\s*\(([^)]*)\)\s*;", src, re.M):
        params = [p.strip() for p in params.split(",")]
        functions[name] = (spell(ret), [] if params == ["void"] else
                           [spell(re.match(r"(.+?)\w+$", p, re.S).group(1)) for p in params])
    struct_fields = {name: sum(d.count(",") + 1 for d in body.split(";") if d.strip())
                     for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", src, re.S)}
    constants = {name: int(val, 0) for name, val in re.findall(r"^#define (F16\w+)\s+(0x[0-9a-fA-F]+|\d+)\s*$", src, re.M)}
    for body in re.findall(r"\benum \w+ \{(.*?)\};", src, re.S):
        val = -1
        for item in filter(None, (x.strip() for x in body.split(","))):
            name, _, given = (x.strip() for x in item.partition("="))
            val = int(given, 0) if given else val + 1
            constants[name] = val
    return {"functions": functions, "struct_fields": struct_fields, "constants": constants}


def struct_layouts(structs, tmp_path):
    """sizeof, and offsetof / size of every field the mirrors name, as the C compiler lays
    include/f16env.h out: {struct: {"sizeof": n, "fields": {field: (offset, size)}}}."""
    lines = ['#include <stdio.h>', '#include "f16env.h"', "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append('printf("%s sizeof %%zu 0\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f, cname, f, cname, f)
                  for f, *_ in mirror._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["return 0; }"]) + "\n")
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    out = {cname: {"fields": {}} for cname in structs}
    for cname, field, a, b in (ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                   check=True).stdout.splitlines()):
        if field == "sizeof":
            out[cname]["sizeof"] = int(a)
        else:
            out[cname]["fields"][field] = (int(a), int(b))
    return out


C_SCALARS = {"int": ("int", 4, True), "int32_t": ("int", 4, True), "uint32_t": ("int", 4, False),
             "int64_t": ("int", 8, True), "uint64_t": ("int", 8, False), "uint8_t": ("int", 1, False),
             "size_t": ("int", ctypes.sizeof(ctypes.c_size_t), False), "double": ("double",), "float": ("float",)}


def c_class(t, structs):
    """Class and width of a C type of the header: ("int", bytes, signed), ("double",), ("str",) for
    the const char* returns, ("ptr", pointee) with pointee a struct's name, a class, or None (void)."""
    if t == "char*":
        return ("str",)
    if t == "f16env_t":  # the opaque handle
        return ("ptr", None)
    if t.endswith("*"):
        base = t[:-1]
        return ("ptr", base if base in structs else None if base == "void" else c_class(base, structs))
    return C_SCALARS[t]


def py_class(t, structs):
    """The same for a ctypes type (c_uint64 and c_size_t are one object here: compared by size and
    signedness, not identity)."""
    if t is ctypes.c_char_p:
        return ("str",)
    if t is ctypes.c_void_p:
        return ("ptr", None)
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        names = {mirror: cname for cname, mirror in structs.items()}
        return ("ptr", names[t._type_] if t._type_ in names else py_class(t._type_, structs))
    if isinstance(t, type) and issubclass(t, ctypes.Structure):
        return ("struct", t.__name__)  # (a mirror that abi.STRUCTS does not name, or one passed by value)
    if t in (ctypes.c_double, ctypes.c_float):
        return ("double",) if t is ctypes.c_double else ("float",)
    return ("int", ctypes.sizeof(t), t(-1).value < 0)


def _agree(c, py):
    """A struct pointer must be a POINTER to its mirror; any other pointer may be void* or a
    POINTER to the pointee's own class; everything else must be the same class and width."""
    if c[0] == "ptr" and py[0] == "ptr" and not isinstance(c[1], str):
        return py[1] is None or py[1] == c[1]
    return c == py


def abi_mismatches(header, layouts, signatures, structs):
    """Every disagreement between the header (parse_header, struct_layouts) and the binding
    (a table like _lib.SIGNATURES, mirrors like abi.STRUCTS), one line each; [] when they agree."""
    bad = []
    protos = header["functions"]
    bad += ["%s: in the table, not in the header" % n for n in signatures if n not in protos]
    bad += ["%s: in the header, not in the table" % n for n in protos if n not in signatures]
    for name in (n for n in signatures if n in protos):
        (ret, params), (restype, argtypes) = protos[name], signatures[name]
        if not _agree(c_class(ret, structs), py_class(restype, structs)):
            bad.append("%s: returns %s, restype %s" % (name, ret, restype.__name__))
        if len(params) != len(argtypes):
            bad.append("%s: %d parameters, %d argtypes" % (name, len(params), len(argtypes)))
        bad += ["%s: parameter %d is %s, argtype %s" % (name, i, c, py.__name__)
                for i, (c, py) in enumerate(zip(params, argtypes))
                if not _agree(c_class(c, structs), py_class(py, structs))]
    for cname, mirror in structs.items():
        if cname not in header["struct_fields"]:
            bad.append("%s: not a struct of the header" % cname)
            continue
        if header["struct_fields"][cname] != len(mirror._fields_):
            bad.append("%s: %d fields in the header, %d in the mirror" % (cname, header["struct_fields"][cname],
                                                                         len(mirror._fields_)))
        if layouts[cname]["sizeof"] != ctypes.sizeof(mirror):
            bad.append("%s: sizeof %d, mirror %d" % (cname, layouts[cname]["sizeof"], ctypes.sizeof(mirror)))
        for f, *_ in mirror._fields_:
            d = getattr(mirror, f)
            if layouts[cname]["fields"].get(f) != (d.offset, d.size):
                bad.append("%s.%s: (offset, size) %s, mirror %s" % (cname, f, layouts[cname]["fields"].get(f),
                                                                    (d.offset, d.size)))
    bad += ["%s: a struct of the header without a mirror" % n for n in header["struct_fields"] if n not in structs]
    return bad


@pytest.fixture(scope="module")
def so_path():
    from f16_jsb_amd.build import build
    return build()


def test_library_exports_every_declared_symbol(so_path):
    out = subprocess.run(["nm", "-D", "--defined-only", so_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (f16env_\w+)", out))
    missing = [f for f in declared_functions() if f not in exported]
    assert not missing, missing


def test_library_loads_without_gpu(so_path):
    from f16_jsb_amd import _lib
    L = _lib.lib()  # imports torch first, then dlopens libf16env.so
    for name in declared_functions():
        assert hasattr(L, name)
    assert set(_lib.EXPORTED_SYMBOLS) == set(declared_functions())
    for name, (restype, argtypes) in _lib.SIGNATURES.items():  # the one loop bound every entry as the table says
        assert getattr(L, name).restype is restype and tuple(getattr(L, name).argtypes) == tuple(argtypes), name
        assert _lib.fn(name) is getattr(L, name)
    with pytest.raises(_lib.F16EnvError, match="has no f16env_nonesuch: rebuild it"):
        _lib.fn("f16env_nonesuch")
    # pure functions need no device
    assert L.f16env_step_kernel_name(None) == b""  # no handle, no kernel
    s = L.f16env_state_bytes_per_env()
    assert 200 <= s <= 400
    assert L.f16env_algorithmic_bytes_per_env_step(4) == 16 + 60 * 4 + 60 * 3 + 4 + 2 + 2 * s
    # the windowed step's moved bytes (bench.py's roofline basis): the state read whole, written
    # back without its per-episode column (goal, episode count) except by the lanes it reset
    from f16_jsb_amd.abi import algorithmic_bytes_per_env_step
    assert algorithmic_bytes_per_env_step(4, s, "window") == 16 + 2 * 60 + 4 + 2 + s + (s - 16)
    assert algorithmic_bytes_per_env_step(10, 256, "window") == 638
    assert algorithmic_bytes_per_env_step(4, 256) == 954  # SURVEY 8(d)'s B(4), the contract


def test_config_default_matches_python_mirror(so_path):
    from f16_jsb_amd import _lib
    from f16_jsb_amd.abi import EnvConfig, config_default
    c = EnvConfig()
    assert _lib.lib().f16env_config_default(ctypes.byref(c)) == 0
    p = config_default()
    for f, _ in EnvConfig._fields_:
        a, b = getattr(c, f), getattr(p, f)
        if f in ("ic", "ic_lo", "ic_hi"):
            assert list(a) == list(b), f
        else:
            assert a == b, f


def test_header_enums_match_python_mirror():
    from f16_jsb_amd import abi
    src = open(HDR).read()
    for name, val in re.findall(r"\b(F16C_\w+)\s*=\s*(\d+)", src):
        assert getattr(abi, name) == int(val), name
    ic_names = re.findall(r"^\s+(F16_IC_\w+)\s*[,=]", src, re.M)
    assert [getattr(abi, n) for n in ic_names] == list(range(len(ic_names)))
    for name, val in re.findall(r"#define (F16_FLAG_\w+)\s+(0x[0-9a-fA-F]+)", src):
        assert getattr(abi, name) == int(val, 16), name
    assert f"#define F16ENV_ABI_VERSION {abi.F16ENV_ABI_VERSION}" in src
    assert abi.F16_IC_N == 19 and abi.F16C_N == 75
    assert "#define F16_OBS_DIM 15" in src


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    from f16_jsb_amd import abi
    return struct_layouts(abi.STRUCTS, tmp_path_factory.mktemp("abi_layout"))


def test_binding_table_matches_header(layouts):
    """Every prototype of include/f16env.h against _lib.SIGNATURES (return type; count, class and
    width of every parameter; struct pointers to their mirrors), the table in the header's order
    with nothing missing on either side, and the four structs' sizeof, field count and every
    field's offset and size against what the C compiler makes of the header."""
    from f16_jsb_amd import _lib, abi
    header = parse_header()
    assert len(header["functions"]) == len(declared_functions()) and len(header["struct_fields"]) == 4
    assert abi_mismatches(header, layouts, _lib.SIGNATURES, abi.STRUCTS) == []
    assert list(_lib.SIGNATURES) == list(header["functions"])
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib.SIGNATURES)
    assert all(isinstance(a, tuple) for _, a in _lib.SIGNATURES.values())


def test_binding_check_reports_wrong_tables(layouts):
    """The comparison on deliberately wrong copies: a parameter dropped, an int64_t bound as 32
    bits, a struct field removed, an entry the header lacks and a prototype the table lacks are
    each reported (and nothing else is)."""
    from f16_jsb_amd import _lib, abi
    header = parse_header()
    i32, i64 = ctypes.c_int32, ctypes.c_int64

    def report(signatures=_lib.SIGNATURES, structs=abi.STRUCTS):
        return abi_mismatches(header, layouts, signatures, structs)
    restype, args = _lib.SIGNATURES["f16env_step"]
    assert report(dict(_lib.SIGNATURES, f16env_step=(restype, args[:-1]))) == ["f16env_step: 13 parameters, 12 argtypes"]
    restype, args = _lib.SIGNATURES["f16env_poses"]
    assert args[1] is i64
    assert report(dict(_lib.SIGNATURES, f16env_poses=(restype, (args[0], i32) + args[2:]))) == \
        ["f16env_poses: parameter 1 is int64_t, argtype c_int"]
    assert report(dict(_lib.SIGNATURES, f16env_poses=(ctypes.c_char_p, args))) == \
        ["f16env_poses: returns int, restype c_char_p"]
    assert report(dict(_lib.SIGNATURES, f16env_create=(restype, (ctypes.POINTER(abi.PolicyDesc),) +
                                                       _lib.SIGNATURES["f16env_create"][1][1:]))) == \
        ["f16env_create: parameter 0 is f16env_config*, argtype LP_PolicyDesc"]

    class ShortSlot(ctypes.Structure):  # RolloutSlot without next_start
        _fields_ = [f for f in abi.RolloutSlot._fields_ if f[0] != "next_start"]
    got = report(structs=dict(abi.STRUCTS, f16env_rollout_slot=ShortSlot))
    assert "f16env_rollout_slot: 10 fields in the header, 9 in the mirror" in got
    assert "f16env_rollout_slot: sizeof 72, mirror 64" in got
    assert "f16env_rollout_slot.features: (offset, size) (48, 8), mirror (40, 8)" in got
    # (the table's POINTER(RolloutSlot) no longer points to the slot's mirror: those two entries are reported too)
    assert {line.split(":")[0].split(".")[0] for line in got} == {"f16env_rollout_slot", "f16env_step_rollout",
                                                                  "f16env_window_step_rollout"}
    assert report(dict(_lib.SIGNATURES, f16env_nonesuch=(i32, ()))) == ["f16env_nonesuch: in the table, not in the header"]
    less = {n: v for n, v in _lib.SIGNATURES.items() if n != "f16env_gae"}
    assert report(less) == ["f16env_gae: in the header, not in the table"]
    # a field added to the header alone: the count differs although every mirrored field still fits
    src = header_source()
    more = src.replace("const float* actions;\n} F16RolloutView;", "const float* actions;\n  const float* extra;\n} F16RolloutView;")
    assert more != src
    assert abi_mismatches(parse_header(more), layouts, _lib.SIGNATURES, abi.STRUCTS) == \
        ["F16RolloutView: 13 fields in the header, 12 in the mirror"]


def test_header_constants_match_python_mirror():
    """Every numeric #define F16* and every enumerator of the header equals the abi attribute of
    the same name (F16_SLOT_*, F16_STEP_*, F16_POLICY_*, F16_PPO_* and the latch enum included),
    and PPO_HYPER / PPO_STATS are the header's order and lengths."""
    from f16_jsb_amd import abi
    constants = parse_header()["constants"]
    # every #define F16* that carries a value was parsed: one spelled (1u << 3) or 0x1u would otherwise go uncompared
    valued = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(F16\w+)[ \t]+\S", header_source(), re.M)
    assert len(valued) >= 33 and [n for n in valued if n not in constants] == []
    assert len(constants) > 100 and {"F16_SLOT_CLIP", "F16_STEP_POSES", "F16_POLICY_OFF_LOG_STD", "F16_PPO_N_STATS",
                                     "F16L_N", "F16C_N", "F16_IC_N", "F16ENV_ABI_VERSION"} <= set(constants)
    assert {n: getattr(abi, n, None) for n in constants} == constants
    hyper = {v: n[len("F16_PPO_HYPER_"):].lower() for n, v in constants.items() if n.startswith("F16_PPO_HYPER_")}
    assert tuple(hyper[i] for i in range(len(hyper))) == abi.PPO_HYPER
    assert len(abi.PPO_HYPER) == constants["F16_PPO_N_HYPER"] and len(abi.PPO_STATS) == constants["F16_PPO_N_STATS"]


def test_create_without_gpu_fails_loudly(so_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd._lib import F16EnvError
    with pytest.raises(F16EnvError):
        F16Envs(4)


def test_null_handle_calls_return_errors(so_path):
    """Every handle-taking entry point of the windowed / features ABI refuses a NULL handle or
    a bad argument with a negative status and a message (no device needed, nothing launched)."""
    from f16_jsb_amd import _lib
    L = _lib.lib()
    assert L.f16env_set_window_order(None, 1) < 0
    assert L.f16env_window_bind(None, None, None, 8, None, None, None, None, None) < 0
    assert L.f16env_window_step_bound(None, None, None, 0, 3) < 0
    assert L.f16env_step_window_nt(None) == -1
    assert L.f16env_step_window_waves_per_simd(None) == 0
    assert L.f16env_step_window(None, None, None, None, None, 8, 3, None, None, None, None, None, None, None) < 0
    assert L.f16env_profile_times(None, None, 4) < 0
    assert L.f16env_window_restart(None, None, None, None, 8, 7) < 0
    assert L.f16env_reset_window(None, None, None, None, None, None, 8, 3) < 0
    # ABI 6
    assert L.f16env_window_resets_deferred(None) < 0
    assert L.f16env_sample_actions_steps(None, None, 1, 0, 4, None) < 0
    # features on a strided block: bad shapes / strides are refused before any launch
    assert L.f16env_features_strided(None, 4, 0, None, 16, 16, None) < 0
    assert L.f16env_features_strided(None, 4, 2, None, -1, 16, None) < 0
    assert L.f16env_features_strided(None, 0, 2, None, 16, 16, None) == 0  # empty: nothing to do
    assert L.f16env_last_error()


def test_product_never_imports_oracle(so_path):
    """No code path of the product reaches the oracle: no Python import of it, no #include
    of oracle/ sources, and libf16env.so does not link it."""
    pkg = os.path.join(ROOT, "f16_jsb_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            txt = open(os.path.join(dp, f), errors="ignore").read() if f.endswith((".py", ".hip", ".h")) else ""
            assert not re.search(r"^\s*(import|from)\s+\S*oracle", txt, re.M), f
            assert not re.search(r"#include\s+\S*oracle", txt), f
            assert "f16ref_" not in txt, f
    needed = subprocess.run(["readelf", "-d", so_path], capture_output=True, text=True).stdout
    assert "f16ref" not in needed


def test_spaces_match_reference_bounds():
    from f16_jsb_amd import spaces
    obs = spaces.observation_space(10)
    assert obs.shape == (10, 15) and obs.dtype == np.float32
    assert obs.low[0, 3] == 0 and obs.high[0, 4] == np.float32(np.pi + 1e-5)
    assert obs.low[0, 10] == np.float32(-np.pi / 2 - 1e-5)
    act = spaces.action_space()
    np.testing.assert_array_equal(act.low, [-1, -1, -1, 0])
    np.testing.assert_array_equal(act.high, [1, 1, 1, 1])


def test_build_deps_are_the_files_the_translation_unit_includes():
    """build.DEPS decides when a library is stale, so it must name every project file the one
    translation unit reads -- no more, no fewer: the compiler's own dependency list (host pass,
    paths under the repository) equals it. And f16env.hip is the host side only: every kernel
    is in a header of its subject (source map)."""
    from f16_jsb_amd import build

    src = os.path.join(ROOT, "f16_jsb_amd", "csrc", "f16env.hip")
    mm = subprocess.run([build.hipcc(), "-MM", "--cuda-host-only", "-I", os.path.join(ROOT, "include"), src],
                        capture_output=True, text=True, check=True).stdout
    words = mm.replace("\\\n", " ").split()[1:]  # (behind the "f16env.o:" target)
    included = {os.path.realpath(w) for w in words}
    included = {w for w in included if w.startswith(os.path.realpath(ROOT) + os.sep)}
    deps = {os.path.realpath(d) for d in build.DEPS}
    assert included == deps, (sorted(included - deps), sorted(deps - included))
    assert "__global__" not in open(src).read()

