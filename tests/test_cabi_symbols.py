"""The C-ABI library loads and exports every entry point include/mrcal_amd.h
declares. No compute calls: runs without a GPU."""
import ctypes
import os
import re

from conftest import ROOT


def declared_functions():
    text = open(os.path.join(ROOT, "include", "mrcal_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(_?mrcal_[A-Za-z0-9_]+)\s*\(", text))
    # typedef'd struct names are not functions
    return sorted(n for n in names if not n.endswith("_t"))


def prototypes():
    """[(return type, name, [parameter, ...])] of include/mrcal_amd.h: every 'type name(parameters);' that is left once
    the comments and the preprocessor lines are gone. No prototype takes a function pointer"""
    text = open(os.path.join(ROOT, "include", "mrcal_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    out = []
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?[\s\*])(\w+)\s*\(([^()]*)\)\s*;", text):
        parameters = m.group(3).strip()
        out.append((m.group(1).strip(), m.group(2), [] if parameters in ("", "void") else [a.strip() for a in parameters.split(",")]))
    return out


_BY_VALUE = {"int": "c_int", "mrcal_lensmodel_type_t": "c_int", "bool": "c_bool", "double": "c_double", "float": "c_float",
             "size_t": "c_size_t", "int64_t": "c_int64", "long": "c_long", "long long": "c_longlong", "uint16_t": "c_uint16",
             "mrcal_problem_selections_t": "ProblemSelections", "mrcal_stats_t": "Stats", "void": None}


def kind_in_header(declaration, is_parameter):
    """'pointer', or what ctypes must say for this C type passed by value"""
    d = re.sub(r"\b(const|struct|restrict|__restrict__)\b", " ", declaration)
    if "*" in d or "[" in d:
        return "pointer"
    words = d.split()
    if is_parameter and " ".join(words) not in _BY_VALUE:
        words = words[:-1]                  # (the parameter's name)
    return getattr(ctypes, _BY_VALUE[" ".join(words)], _BY_VALUE[" ".join(words)]) if _BY_VALUE[" ".join(words)] else None


def kind_in_table(ctype):
    from mrcal_amd import _cabi
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
        return "pointer"
    return {_cabi.ProblemSelections: "ProblemSelections", _cabi.Stats: "Stats"}.get(ctype, ctype)


def table_against_header(signatures, debug_signatures=()):
    """every disagreement between the header and a table of signatures, as text"""
    wrong = []
    declared = {name: (ret, parameters) for ret, name, parameters in prototypes()}
    for name, (ret, parameters) in declared.items():
        if name not in signatures:
            wrong.append(f"{name}: no row")
            continue
        restype, argtypes = signatures[name]
        if kind_in_table(restype) != kind_in_header(ret, False):
            wrong.append(f"{name}: returns '{ret}', the table says {restype}")
        if len(argtypes) != len(parameters):
            wrong.append(f"{name}: {len(parameters)} parameters, the table has {len(argtypes)}")
            continue
        for i, (parameter, argtype) in enumerate(zip(parameters, argtypes)):
            if kind_in_table(argtype) != kind_in_header(parameter, True):
                wrong.append(f"{name}: parameter {i} is '{parameter}', the table says {argtype}")
    wrong += [f"{name}: a row, and not in the header" for name in signatures if name not in declared]
    wrong += [f"{name}: marked as a debug entry point, and in the header" for name in debug_signatures if name in declared]
    return wrong


def test_prototypes_are_all_found():
    found = prototypes()
    assert len(found) == 221
    assert sorted(name for _, name, _ in found) == declared_functions()


def test_signature_table_agrees_with_the_header():
    """_cabi.SIGNATURES, the one place where the Python side says what the C functions take, against the header:
    a row for every prototype and no other, the same number of arguments, and the same kind of value each"""
    from mrcal_amd._cabi import SIGNATURES, DEBUG_SIGNATURES
    wrong = table_against_header(SIGNATURES, DEBUG_SIGNATURES)
    assert not wrong, "\n".join(wrong)
    lib = ctypes.CDLL(os.path.join(ROOT, "mrcal_amd", "libmrcal_amd.so"))
    missing = [n for n in list(SIGNATURES) + list(DEBUG_SIGNATURES) if not hasattr(lib, n)]
    assert not missing, f"in the table but not exported: {missing}"


def test_signature_check_sees_a_wrong_row():
    """the comparison itself: a c_int where the header says size_t, a missing pointer, a missing argument and a missing
    row are each reported"""
    from mrcal_amd._cabi import SIGNATURES
    name = "mrcal_amd_chessboard_detector_create"
    restype, argtypes = SIGNATURES[name]
    for row, what in (((restype, argtypes[:-1] + [ctypes.c_int]), "parameter 4"),
                      ((ctypes.c_int, argtypes), "returns"),
                      ((restype, argtypes[:-1]), "5 parameters")):
        wrong = table_against_header(dict(SIGNATURES, **{name: row}))
        assert len(wrong) == 1 and wrong[0].startswith(name) and what in wrong[0], wrong
    assert table_against_header({k: v for k, v in SIGNATURES.items() if k != name}) == [f"{name}: no row"]


def test_no_signature_outside_the_table():
    """no module of the package but _cabi.py sets a restype or argtypes"""
    import glob
    for path in glob.glob(os.path.join(ROOT, "mrcal_amd", "*.py")):
        if os.path.basename(path) != "_cabi.py":
            assert not re.search(r"restype|argtypes", open(path).read()), path


def test_header_declares_something():
    names = declared_functions()
    assert "mrcal_optimize" in names
    assert "mrcal_optimizer_callback" in names
    assert "mrcal_amd_problem_create" in names
    assert len(names) > 40


def test_every_declared_symbol_is_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "mrcal_amd", "libmrcal_amd.so"))
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, f"declared in include/mrcal_amd.h but not exported: {missing}"


def test_no_gpu_means_loud_failure(amd):
    """the product has no CPU fallback"""
    import numpy as np
    import pytest
    if amd.gpu_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        amd.optimizer_callback(intrinsics = np.array(((1000.,1000.,500.,500.),)),
                               lensmodel = "LENSMODEL_PINHOLE",
                               imagersizes = np.array(((1000,1000),), dtype=np.int32),
                               rt_ref_frame = np.array(((0.,0,0,0,0,2.),)),
                               observations_board = np.ones((1,3,3,3)),
                               indices_frame_camintrinsics_camextrinsics = np.array(((0,0,-1),), dtype=np.int32),
                               calibration_object_spacing = 0.1,
                               do_optimize_calobject_warp = False)
    # the half-made problem was deleted on the spot: nothing of it is held
    assert amd._lib.lib.mrcal_amd_device_buffers_live() == 0
