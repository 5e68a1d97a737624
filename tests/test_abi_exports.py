"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol
include/slam_engine.h declares (no compute calls without a GPU)."""
import ctypes as C
import os

from slamkit_amd import engine as E


def test_library_exports_every_declared_symbol():
    lib = E.load_library()
    names = E.header_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/slam_engine.h but not exported"
    # and the binding covers exactly the declared functions
    assert sorted(lib._slam_signatures) == names


def _type_name(t):
    return "void" if t is None else "BUCKET_CB" if t is E.BUCKET_CB else t.__name__


def test_derived_signatures_equal_the_hand_written_table():
    """The bindings read from include/slam_engine.h equal, entry for entry, the table load_library used to restate by hand:
    tests/golden/abi_signatures.json is that table's _slam_signatures (ctypes class names), frozen when the table was deleted.
    It proves that deletion and is no second source of truth: a pull request that changes the header regenerates it from
    lib._slam_signatures with _type_name above."""
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_signatures.json")) as f:
        frozen = json.load(f)
    got = {n: [_type_name(r), [_type_name(a) for a in args]] for n, (r, args) in E.load_library()._slam_signatures.items()}
    assert len(frozen) == 177 and sorted(got) == sorted(frozen)
    for n in frozen:
        assert got[n] == frozen[n], n
    # the override table holds the functions with a typed scalar pointer (the host out-parameters) and nothing else
    typed = {n for n, (_, args) in frozen.items() if any(a.startswith("LP_c_") and a != "LP_c_void_p" for a in args)}
    assert typed == set(E._HOST_OUT) and len(typed) == 6


def test_header_reader_on_synthetic_headers():
    import pytest
    # a prototype over three lines; a comment and the callback typedef that only look like functions; void and struct pointers
    fns, defines, structs = E._parse_header(
        "#ifndef X_H\n#define X_H\n#define SLAM_A 7\n#define SLAM_B (-3)   /* slam_no( */\n#define SLAM_NOT_INT 1.5\n"
        "/* int slam_foo(int x); */\ntypedef struct SlamEngine SlamEngine;\n"
        "typedef void (*slam_bucket_cb)(void* user, int64_t offset, int64_t count);\n"
        "typedef struct SlamPair { int64_t a, b; char tag[8]; float* p; } SlamPair;\n"
        "const char* slam_three(SlamEngine* h, const SlamWarpDesc* w,\n     const int64_t ids[],\n"
        "     slam_bucket_cb cb, SlamEngine** out, const SlamPair* unmirrored, size_t n);\n"
        "void slam_none(void);\n#endif\n")
    assert fns == {"slam_three": (C.c_char_p, [C.c_void_p, C.POINTER(E.SlamWarpDesc), C.c_void_p, E.BUCKET_CB, C.POINTER(C.c_void_p),
                                               C.c_void_p, C.c_size_t]),
                   "slam_none": (None, [])}
    assert defines == {"SLAM_A": 7, "SLAM_B": -3}
    assert structs == {"SlamPair": [("a", C.c_int64), ("b", C.c_int64), ("tag", C.c_char * 8), ("p", C.c_void_p)]}
    # a type the rule does not know is an error that names the function, never a default
    with pytest.raises(TypeError, match="slam_bad, parameter 1.*'uint16_t'"):
        E._parse_header("int slam_ok(int a);\nint slam_bad(int a, uint16_t b);\n")
    with pytest.raises(TypeError, match="slam_worse, return type"):
        E._parse_header("long slam_worse(int a);\n")
    with pytest.raises(TypeError, match="slam_two_words, parameter 0"):
        E._parse_header("int slam_two_words(unsigned int a);\n")
    with pytest.raises(TypeError, match="cannot read"):
        E._parse_header("int slam_fnptr(void (*cb)(int));\n")


def test_struct_mirrors_match_the_header():
    """Every struct of include/slam_engine.h with a body, parsed by the rule that types the functions, is mirrored in engine.py
    by a ctypes.Structure of the same field names, order and types (arrays as type * n)."""
    assert len(E._STRUCTS) == 8
    for name, fields in E._STRUCTS.items():
        cls = getattr(E, name)
        assert issubclass(cls, C.Structure) and list(cls._fields_) == fields, name
    mirrors = {n for n, v in vars(E).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert mirrors == set(E._STRUCTS)


def _defined_dynamic_symbols(path):
    """Names in the dynamic symbol table of `path` that the library itself defines: nm -D, or ROCm's llvm-readelf."""
    import shutil
    import subprocess
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}
    readelf = shutil.which("llvm-readelf") or next(
        (p for p in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), d, "llvm-readelf") for d in ("llvm/bin", "lib/llvm/bin", "bin"))
         if os.path.exists(p)), None)
    assert readelf, "neither nm nor llvm-readelf found: the exported symbols cannot be read"
    out = subprocess.run([readelf, "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
    syms = set()
    for ln in out.splitlines():  # Num: Value Size Type Bind Vis Ndx Name
        f = ln.split()
        if len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit() and f[6] != "UND" and f[3] != "SECTION":
            syms.add(f[7].split("@")[0])
    return syms


def test_library_exports_nothing_but_the_declared_abi():
    """The dynamic symbol table of libslam_engine.so (and of the probes build, where it has been built) is the set of functions
    include/slam_engine.h declares, exactly: no internal launcher, no SlamEngine member, no C++ runtime instantiation that a
    consumer's own symbols could preempt or share (csrc/exports.map)."""
    from slamkit_amd.csrc import build as B
    declared = set(E.header_symbols())
    assert os.path.exists(B.LIB), B.LIB
    for path in (B.LIB, B.PROBES_LIB):
        if not os.path.exists(path):
            continue
        got = _defined_dynamic_symbols(path)
        assert got == declared, (path, sorted(got - declared)[:20], sorted(declared - got)[:20])


def test_engine_layout_without_gpu():
    lib = E.load_library()
    assert b"gfx950" in lib.slam_version()
    d = E.SlamModelDesc(24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
    eng = E.Engine(d)
    # 358,347,904 reference parameters + 10 zero pad rows of the 512-row embedding image
    assert eng.n_params == 358_347_904 + 10 * 896
    t = eng.tensors
    assert t["embed"].rows == 512 and t["embed"].offset == 0
    assert t["layers.0.wqkv"].rows == 1152 and t["layers.0.wgu"].rows == 9728
    assert all(s.offset % 8 == 0 for s in t.values())
    assert eng.workspace_bytes(8192) > 7 * 2**30
    # bad descriptions are rejected with an error code, not a crash
    h = C.c_void_p()
    bad = E.SlamModelDesc(2, 100, 4, 2, 32, 512, 502, 0, 1e-6, 10000.0)
    assert lib.slam_engine_create(C.byref(bad), C.byref(h)) == -1
    assert lib.slam_backward(None, 1.0, 0, E.BUCKET_CB(0), None, None) == -1
    eng.close()


def test_missing_library_fails_loudly(tmp_path):
    import pytest
    with pytest.raises(OSError):
        E.load_library(str(tmp_path / "nope.so"))


def test_gemm_tn_workspace_covers_every_contraction_length():
    """The wgrad planners re-plan from the runtime token count (packed micro-batches vary): the workspace sized for Mmax must
    cover the plan of every M <= Mmax (round-2 advisor finding: H 256, I 1024, Mmax 2048 - at M = 1600 the gate|up plan
    needed 10.0 MiB of an 8.0 MiB allocation). Host-only: the sizing function does not touch the device."""
    from slamkit_amd import engine as E
    lib = E.load_library()
    assert lib.slam_op_gemm_tn_workspace(2048, 2048, 256) >= 10 * 2 ** 20
    for N, K in ((2048, 256), (9728, 896), (896, 4864), (1152, 896), (896, 896)):
        cap = lib.slam_op_gemm_tn_workspace(8192, N, K)
        for M in range(64, 8192 + 1, 64):
            assert lib.slam_op_gemm_tn_workspace(M, N, K) <= cap, (M, N, K)


def test_c_consumer_compiles_against_the_header(tmp_path):
    """include/slam_engine.h is plain C and tools/examples/c_dp_consumer.c - one data-parallel optimizer step of a consumer without
    torch: forward, backward with the bucket callback calling slam_allreduce_grads_async, slam_comm_finish, clip, AdamW - still
    matches it (compile only: gcc, C99, warnings as errors)."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        import pytest
        pytest.skip("no C compiler on this box")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), "-c",
                        os.path.join(root, "tools", "examples", "c_dp_consumer.c"), "-o", str(tmp_path / "c.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_product_library_cannot_skip_output_stores():
    """Round-5 verdict / advisor: bit 1 of gemm_nt_store made every NT GEMM drop its output stores and was reachable from the
    environment (SLAM_GEMM_NT_STORE). It is compiled out of the product library now (-DSLAM_PROBES builds only): the option is
    rejected beyond {0, 1}, for the process default and for an engine, and UnitLM no longer forwards it from the environment.
    Host-only calls."""
    lib = E.load_library()
    assert lib.slam_set_option(None, b"gemm_nt_store", 2) == -1
    assert lib.slam_set_option(None, b"gemm_nt_store", 3) == -1
    assert lib.slam_set_option(None, b"gemm_nt_store", 1) == 0
    assert lib.slam_set_option(None, b"gemm_nt_store", 0) == 0
    eng = E.Engine(E.SlamModelDesc(2, 64, 4, 2, 64, 128, 502, 0, 1e-6, 10000.0))
    import pytest
    with pytest.raises(E.EngineError, match="out of range"):
        eng.set_option("gemm_nt_store", 2)
    eng.set_option("gemm_nt_store", 0)
    with pytest.raises(E.EngineError):
        eng.set_option("grad_final_next", 3)
    eng.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "gemm_nt_store" not in open(os.path.join(root, "slamkit_amd", "model", "unit_lm.py")).read()
    src = open(os.path.join(root, "slamkit_amd", "csrc", "build.py")).read()
    assert "-DSLAM_PROBES" in src and "libslam_engine_probes.so" in src


def test_address_arithmetic_of_the_32x32x16_gemm_paths():
    """tools/layout_sim.py: the index arithmetic of gemm.hip's 32x32x16 main loops restated on labels - LDS-DMA placement ->
    swizzled fragment reads -> MFMA lane maps -> epilogue32 columns - for the 128 x 128, the eight-wave 256 x 256 and the four-wave
    256 x 256 kernel: every stored element is the product sum it should be, every ds_read_b128 lane group is conflict-free."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("layout_sim", os.path.join(root, "tools", "layout_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.sim_128x128()
    m.sim_256_8wave()
    m.sim_256_4wave()
