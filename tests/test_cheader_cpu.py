"""CPU-only checks of vss_amd/cheader.py, the parser the ctypes binding is derived with: every form include/vss.h
uses on small synthetic headers, every case it must refuse, the real header's struct layouts against the C
compiler's, and the oracle's hand-kept mirrors against the derived ones."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from vss_amd import _native as N
from vss_amd import cheader

P = C.c_void_p


def functions(text):
    return cheader.parse(text).functions


def test_prototype_forms():
    f = functions("""
        int vss_a(void);
        const char* vss_b(int code);
        int64_t vss_c(void* stream, int64_t rows,
                      int32_t cols, const float* x,
                      uint64_t seed, uint32_t call, float g, double n);
        int vss_d(void* stream, const float* obs, const float* term /* NULL: start, (a, b) */,
                  float* ring /* (delay+1, n) */, int32_t* age);  /* trailing */
        int vss_e(const float* const* w, uint16_t* const* w_split, const uint32_t ctr[4], uint32_t out[4]);
        void vss_f(const vss_params* p, int32_t);   // a struct by pointer, an unnamed scalar
        float vss_g(float x);
        const char * vss_h ( void ) ;
    """)
    assert list(f) == ["vss_a", "vss_b", "vss_c", "vss_d", "vss_e", "vss_f", "vss_g", "vss_h"]
    assert f["vss_a"] == (C.c_int, [])
    assert f["vss_b"] == (C.c_char_p, [C.c_int])
    assert f["vss_c"] == (C.c_int64, [P, C.c_int64, C.c_int32, P, C.c_uint64, C.c_uint32, C.c_float, C.c_double])
    assert f["vss_d"] == (C.c_int, [P, P, P, P, P])
    assert f["vss_e"] == (C.c_int, [P, P, P, P])
    assert f["vss_f"] == (None, [P, C.c_int32])
    assert f["vss_g"] == (C.c_float, [C.c_float])
    assert f["vss_h"] == (C.c_char_p, [])


def test_constants_structs_and_the_cplusplus_guard():
    h = cheader.parse("""
        #ifndef GUARD_H
        #define GUARD_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VSS_N 16   /* a comment */
        #define VSS_HEX 0x10
        #define VSS_NEG -3
        #define VSS_NAME "text"
        #define VSS_EXPR (1 << 4)
        #define VSS_CALL(x) x
        typedef struct vss_s {
          float a;            /* scalar */
          int32_t n;
          uint64_t seed;
          const float* p;     /* pointer */
          uint8_t* q;
          const float* table[VSS_N];
          float* four[4];
          float pos, vel, ang;
          double d;
        } vss_s;
        typedef struct vss_t { float x, y; } vss_t;
        int vss_use(const vss_s* s);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert h.constants == {"VSS_N": 16, "VSS_HEX": 16, "VSS_NEG": -3}
    assert list(h.structs) == ["vss_s", "vss_t"] and list(h.functions) == ["vss_use"]
    s = h.structs["vss_s"]
    assert issubclass(s, C.Structure)
    assert [n for n, _ in s._fields_] == ["a", "n", "seed", "p", "q", "table", "four", "pos", "vel", "ang", "d"]
    types = dict(s._fields_)
    assert (types["a"], types["n"], types["seed"], types["p"], types["q"]) == (C.c_float, C.c_int32, C.c_uint64, P, P)
    assert (types["table"]._type_, types["table"]._length_) == (P, 16)
    assert (types["four"]._type_, types["four"]._length_) == (P, 4)
    assert types["pos"] == types["vel"] == types["ang"] == C.c_float and types["d"] == C.c_double
    assert s.seed.offset == 8 and s.p.offset == 16 and s.table.offset == 32 and C.sizeof(s) == 32 + 20 * 8 + 12 + 4 + 8
    v = h.structs["vss_t"](1.5, 2.5)  # positional construction, as the callers build their structs
    assert (v.x, v.y) == (1.5, 2.5)


@pytest.mark.parametrize("text, names", [
    ("int vss_f(int8_t x);", ["vss_f", "int8_t"]),                                    # a scalar outside the table
    ("int vss_f(unsigned int x);", ["vss_f", "unsigned int"]),
    ("int vss_f(int64_t n, vss_params p);", ["vss_f", "parameter 1", "vss_params"]),   # a struct by value
    ("vss_params vss_f(void);", ["vss_f", "vss_params"]),                              # ... returned by value
    ("float* vss_f(void);", ["vss_f", "float *"]),                                     # a pointer that is no string
    ("int vss_f(int (*cb)(int));", ["vss_f"]),                                         # a function pointer
    ("int vss_f(int x, ...);", ["vss_f", "..."]),
    ("int vss_f(int x);\nint vss_f(int x);", ["vss_f", "twice"]),
    ("static inline int vss_f(int x) { return x; }", ["vss_f"]),                       # not a prototype
    ("int vss_ok(void);\nint vss_g(int x)", ["vss_g"]),                                # an unterminated vss_g(
    ("typedef struct vss_s { int32_t a : 3; } vss_s;", ["vss_s", ":"]),                # a bit-field
    ("typedef struct vss_s { union { int a; float b; } u; } vss_s;", ["vss_s"]),       # a union
    ("typedef struct vss_s { struct { int a; } in; } vss_s;", ["vss_s"]),              # a nested struct
    ("typedef struct vss_s { struct vss_t t; } vss_s;", ["vss_s", "struct"]),
    ("typedef struct vss_s { vss_t t; } vss_s;", ["vss_s.t", "vss_t"]),                # a struct member by value
    ("typedef struct vss_s { uint8_t flag; } vss_s;", ["vss_s.flag", "uint8_t"]),
    ("typedef struct vss_s { float* a, b; } vss_s;", ["vss_s", "float* a, b"]),        # a pointer in a shared declaration
    ("typedef struct vss_s { float a[VSS_UNKNOWN]; } vss_s;", ["vss_s.a", "VSS_UNKNOWN"]),
    ("typedef struct vss_s { float a; } vss_other;", ["vss_s", "vss_other"]),
    ("typedef struct { float a; } vss_s;", ["typedef struct {"]),                                # an anonymous struct
    ("typedef enum vss_e { A, B } vss_e;", ["vss_e"]),
    ("typedef union vss_u { int a; float b; } vss_u;", ["vss_u"]),
])
def test_the_parser_fails_closed(text, names):
    with pytest.raises(cheader.HeaderError) as e:
        cheader.parse(text)
    for name in names:
        assert name in str(e.value), str(e.value)


def test_bind_sets_every_prototype_and_names_a_missing_symbol():
    class Fn:
        restype = argtypes = "unset"

    class Lib:
        vss_a, vss_b = Fn(), Fn()
    h = cheader.parse("int64_t vss_a(void* s, int32_t n);\nconst char* vss_b(void);")
    lib = cheader.bind(Lib(), h)
    assert (lib.vss_a.restype, lib.vss_a.argtypes) == (C.c_int64, [P, C.c_int32])
    assert (lib.vss_b.restype, lib.vss_b.argtypes) == (C.c_char_p, [])
    with pytest.raises(AttributeError, match="vss_c"):
        cheader.bind(Lib(), cheader.parse("int vss_c(void);"))
    with pytest.raises(N.NativeError, match="lacks an entry point"):
        N.bind(Lib())


def test_the_loaded_library_carries_the_headers_types():
    """load() binds through bind(): every entry point of the loaded library has the parsed restype and argtypes, a
    pointer never an integer slot, and the modules' names are the header's values."""
    lib = N.load()
    assert len(N.ABI.functions) == 66 and tuple(N.ABI.functions) == N.EXPORTED
    for name, (restype, argtypes) in N.ABI.functions.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert lib.vss_step.argtypes == [P, C.c_int64, C.c_int32, P, P, P]
    assert lib.vss_gae.argtypes == [P, C.c_int64, C.c_int64] + [P] * 7 + [C.c_float, C.c_float, P, P]
    assert lib.vss_perceive.argtypes == [P, C.c_int64, P, C.c_int32, P, C.c_uint64, C.c_uint32, P, P, P, C.c_int64,
                                         P, P, P, P]
    assert lib.vss_mlp_packed_size.restype == C.c_int64 and lib.vss_error_string.restype == C.c_char_p
    for name, value in N.ABI.constants.items():
        assert getattr(N, name[len("VSS_"):]) == value, name
    assert (N.MODE_FULL, N.MODE_SA, N.MODE_CMA, N.MODE_DMA) == (0, 1, 2, 3)
    assert (N.CH_BALL_X, N.CH_RX, N.CH_RW, N.STATE_CHANNELS) == (0, 4, 52, 58)
    structs = {"vss_params": N.VssParams, "vss_state": N.VssState, "vss_step_io": N.VssStepIO,
               "vss_rollout_io": N.VssRolloutIO, "vss_replay_draws": N.VssReplayDraws, "vss_versus_io": N.VssVersusIO,
               "vss_mirror_io": N.VssMirrorIO, "vss_actor_groups": N.VssActorGroups,
               "vss_perceive_layout": N.VssPerceiveLayout, "vss_perceive_noise": N.VssPerceiveNoise,
               "vss_actuate_layout": N.VssActuateLayout, "vss_actuate_params": N.VssActuateParams,
               "vss_estimate_layout": N.VssEstimateLayout,
               "vss_track_layout": N.VssTrackLayout, "vss_track_params": N.VssTrackParams,
               "vss_setplay_entity": N.VssSetplayEntity, "vss_setplay_play": N.VssSetplayPlay,
               "vss_setplay_table": N.VssSetplayTable, "vss_setplay_view": N.VssSetplayView,
               "vss_referee_play": N.VssRefereePlay, "vss_referee_table": N.VssRefereeTable,
               "vss_referee_params": N.VssRefereeParams}
    assert structs == N.ABI.structs


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    """sizeof and every offsetof of every struct of include/vss.h, printed by a C program that includes the header,
    against the derived ctypes classes."""
    if not shutil.which("gcc"):
        pytest.skip("gcc is not available")
    lines, want = [], []
    for name, cls in N.ABI.structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(cls)}")
        for member, _ in cls._fields_:
            lines.append(f'  printf("{name}.{member} %zu\\n", offsetof({name}, {member}));')
            want.append(f"{name}.{member} {getattr(cls, member).offset}")
        lines.append(f'  printf("{name}.. %zu\\n", sizeof((({name}*)0)->{cls._fields_[-1][0]}));')  # the last member's size
        want.append(f"{name}.. {getattr(cls, cls._fields_[-1][0]).size}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vss.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(N.HEADER), "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(N.ABI.structs) == 22 and got == want


def test_the_oracles_mirrors_equal_the_derived_ones():
    """oracle/oracle.py keeps its own structs and constants (it imports nothing of the product package); they are
    the header's: member names, ctypes types and offsets, and every constant it names."""
    import oracle as O
    for mine, theirs in ((N.VssParams, O.VssParams), (N.VssState, O.VssState), (N.VssStepIO, O.VssStepIO)):
        assert theirs._fields_ == mine._fields_, theirs.__name__
        assert [getattr(theirs, n).offset for n, _ in theirs._fields_] == [getattr(mine, n).offset for n, _ in mine._fields_]
        assert C.sizeof(theirs) == C.sizeof(mine)
    names = [n for n in vars(O) if n.startswith(("MODE_", "CH_")) or n == "STATE_CHANNELS"]
    assert len(names) == 4 + 1 + 10
    for name in names:
        assert getattr(O, name) == getattr(N, "CH_BALL_X" if name == "CH_BALL" else name), name


def test_the_oracles_prototypes_equal_its_header():
    """The parser reads oracle/vss_oracle.h too (void and float returns, array parameters): what oracle.py sets by
    hand on its library is what the header declares."""
    import oracle as O
    with open(os.path.join(os.path.dirname(O.__file__), "vss_oracle.h")) as f:
        h = cheader.parse(f.read().replace('#include "../include/vss.h"', ""))
    assert list(h.structs) == ["oracle_draws"] and h.structs["oracle_draws"]._fields_ == O.OracleDraws._fields_
    assert h.functions["oracle_logf"] == (C.c_float, [C.c_float])
    assert h.functions["oracle_philox"] == (None, [C.c_uint32, C.c_uint32, P, P])
    lib, checked = O.lib(), 0
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)
        if fn.argtypes is not None:
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype == restype or restype is None, name  # oracle.py ignores what a void function returns
            checked += 1
    assert checked == 11
