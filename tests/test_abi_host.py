"""CPU-side checks of the derived ctypes binding (newtonnet_amd/abi.py): the host C++ compiler agrees with the parser on every
function signature, struct size and member offset of include/newtonnet_hip.h; the parser follows the text it is given and refuses
what it does not know; the derived parameter types accept what the call sites pass; everything is declared when the library loads."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from newtonnet_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE_HEAD = r'''
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "newtonnet_hip.h"
template <class T> constexpr char code() {
  return std::is_pointer<T>::value ? 'p' : std::is_same<T, int32_t>::value ? 'i' : std::is_same<T, float>::value ? 'f'
       : std::is_same<T, double>::value ? 'd' : std::is_same<T, size_t>::value ? 'z' : std::is_same<T, int64_t>::value ? 'q'
       : std::is_void<T>::value ? 'v' : '?';
}
template <class R, class... A> void sig(const char* name, R (*)(A...)) {
  const char args[] = {code<A>()..., 0};
  std::printf("F %s %c %s\n", name, code<R>(), args);
}
int main() {
'''


def _code(t):
    if t is None:
        return 'v'
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return 'p'
    return {C.c_int32: 'i', C.c_float: 'f', C.c_double: 'd', C.c_size_t: 'z', C.c_int64: 'q'}[t]


def test_the_compiler_agrees_with_the_parser(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler here')
    lines = [PROBE_HEAD]
    lines += [f'  sig("{f}", static_cast<decltype(&{f})>(nullptr));' for f in abi.FUNCTIONS]
    for s, cls in abi.STRUCTS.items():
        lines.append(f'  std::printf("S {s} %zu\\n", sizeof({s}));')
        lines += [f'  std::printf("M {s} {m} %zu %zu\\n", offsetof({s}, {m}), sizeof({s}::{m}));' for m, _ in cls._fields_]
    lines += [f'  std::printf("K {k} %lld\\n", (long long){k});' for k in abi.CONSTANTS]
    lines.append('  return 0;\n}\n')
    src, exe = tmp_path / 'probe.cpp', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run([cxx, '-std=c++17', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    funcs, sizes, members, consts = {}, {}, {}, {}
    for line in out.splitlines():
        w = line.split(' ')
        if w[0] == 'F':
            funcs[w[1]] = (w[2], w[3])
        elif w[0] == 'S':
            sizes[w[1]] = int(w[2])
        elif w[0] == 'M':
            members[(w[1], w[2])] = (int(w[3]), int(w[4]))
        else:
            consts[w[1]] = int(w[2])
    assert len(funcs) == len(abi.FUNCTIONS) >= 108 and len(sizes) == len(abi.STRUCTS) >= 10 and len(members) >= 257
    assert consts == abi.CONSTANTS and len(consts) >= 30
    assert not any('?' in r + a for r, a in funcs.values())
    for f, (restype, argtypes) in abi.FUNCTIONS.items():
        assert funcs[f] == (_code(restype), ''.join(_code(t) for t in argtypes)), f
    for s, cls in abi.STRUCTS.items():
        assert C.sizeof(cls) == sizes[s], s
        assert len(cls._fields_) == sum(1 for k in members if k[0] == s)
        for m, _ in cls._fields_:
            assert (getattr(cls, m).offset, getattr(cls, m).size) == members[(s, m)], (s, m)
    assert sum(len(cls._fields_) for cls in abi.STRUCTS.values()) == len(members)
    # what hip.py hands out is the derived classes, and a struct pointer is typed wherever the table is host memory
    assert hip.Model is abi.STRUCTS['nnhip_model'] and hip.TrainWs is abi.STRUCTS['nnhip_train_ws']
    assert abi.FUNCTIONS['nnhip_train_values'][1][:2] == [C.POINTER(hip.Model), C.POINTER(hip.TrainWs)]


def test_the_parser_follows_its_text():
    proto = 'typedef struct { int32_t n; } s_t;\nint f(const s_t* s, %s k, const float box[3], float* const* t, void* stream);'
    _, structs, funcs = abi.parse(proto % 'int32_t')
    assert funcs['f'] == (C.c_int32, [C.POINTER(structs['s_t']), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
    assert abi.parse(proto % 'float')[2]['f'][1][1] is C.c_float
    consts, structs, funcs = abi.parse('''
        #define NNHIP_MAX_LAYERS 8   /* a comment */
        #define NNHIP_NEG (-1)
        #define NNHIP_TINY 1e-4f
        enum { A_ = 3, B_, C_ = 0x10 };
        typedef struct { float* a[NNHIP_MAX_LAYERS][7]; } wide_t;
        typedef struct { int32_t a, b; float* c, *d; wide_t w[2]; size_t n; } mixed_t;
        size_t g(void); const char* h(void); int64_t q(double x, int64_t n, const uint8_t* m); void v(int k);''')
    assert consts == {'NNHIP_MAX_LAYERS': 8, 'NNHIP_NEG': -1, 'A_': 3, 'B_': 4, 'C_': 16}
    assert C.sizeof(structs['wide_t']) == 8 * 7 * 8 and structs['wide_t']._fields_[0][1] is (C.c_void_p * 7) * 8
    assert structs['mixed_t']._fields_ == [('a', C.c_int32), ('b', C.c_int32), ('c', C.c_void_p), ('d', C.c_void_p),
                                           ('w', structs['wide_t'] * 2), ('n', C.c_size_t)]
    assert funcs == {'g': (C.c_size_t, []), 'h': (C.c_char_p, []), 'q': (C.c_int64, [C.c_double, C.c_int64, C.c_void_p]),
                     'v': (None, [C.c_int32])}


@pytest.mark.parametrize('text', [
    'typedef struct { real_t x; } s_t;',                       # an unknown type name
    'int f(real_t x);',
    'typedef struct { int (*callback)(int); } s_t;',           # a function-pointer member
    'typedef struct { int32_t a : 3; } s_t;',                  # a bitfield
    'typedef struct { union { int32_t a; float b; } u; } s_t;',
    'typedef union { int32_t a; float b; } u_t;',
    'typedef struct { float* a[NNHIP_UNKNOWN]; } s_t;',        # an extent that is neither a literal nor a known constant
    'typedef struct { float a[2 * 4]; } s_t;',
    'typedef struct { int32_t n; } s_t; int f(s_t by_value);',
    'int f(void x);',
    'int global_variable;',
    '#define NNHIP_TWICE(x) (2 * (x))',
    '#if 1\nint f(void);\n#endif',
    'extern "C" {\nint f(void);',
    'int f(void);\n}',
])
def test_the_parser_refuses_what_it_does_not_know(text):
    with pytest.raises(hip.HipLibraryError, match='no ctypes binding can be derived'):
        abi.parse(text)


def test_derived_types_accept_what_call_sites_pass():
    vp = abi.FUNCTIONS['nnhip_graph_count'][1][0]
    assert vp is C.c_void_p
    model, n = hip.Model(), 3
    for value in (None, 0x7f0000001000, C.c_void_p(0x7f0000001000), (C.c_float * 3)(), (C.c_void_p * n)(), (C.c_double * 14)(),
                  C.create_string_buffer(16), C.byref(model)):
        vp.from_param(value)
    with pytest.raises(TypeError):
        vp.from_param(1.5)
    typed = abi.FUNCTIONS['nnhip_energy_forces'][1][0]
    assert typed is C.POINTER(hip.Model)
    typed.from_param(C.byref(model))
    with pytest.raises(TypeError):
        typed.from_param(C.byref(hip.TrainWs()))
    for name, k in abi.DEVICE_TABLE_PARAMS:            # (their tables are device memory: callers pass tensor.data_ptr())
        assert abi.FUNCTIONS[name][1][k] is C.c_void_p
        abi.FUNCTIONS[name][1][k].from_param(0x7f0000001000)


def test_every_entry_point_is_declared_at_load():
    L = hip.lib()
    assert hip.EXPORTED_SYMBOLS == tuple(abi.FUNCTIONS) and len(hip.EXPORTED_SYMBOLS) >= 108
    for name in hip.EXPORTED_SYMBOLS:
        fn = getattr(L, name)
        restype, argtypes = abi.FUNCTIONS[name]
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype is restype, name
    assert L.nnhip_spatial_order_scratch_bytes.restype is C.c_size_t and L.nnhip_bf16_mlp_launches.restype is C.c_int64
    assert L.nnhip_last_error.restype is C.c_char_p


def test_stage_ex_entry_points_check_their_arguments():
    """the *_ex stage entry points (nnhip_stage_opts) refuse bad arguments before any launch, in the ARG_CHECK style -- the failed
    condition is in the error string -- and zero atoms is NNHIP_OK without a launch (no GPU is touched: the pointers are never
    followed)"""
    L = hip.lib()
    OK, E_INVALID = 0, 1
    p = 0x7f0000001000                        # stands for any device array
    N, E = 99, 1502
    Opts = abi.STRUCTS['nnhip_stage_opts']
    assert abi.FUNCTIONS['nnhip_message_bwd_ex'][1][12] == C.POINTER(Opts) and C.sizeof(Opts) == 72

    def opts(**kw):
        o = Opts()
        o.pair_ptr = o.rev = o.mol_ptr = p
        o.n_mol, o.small_molecules = 7, 1
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def tail(**kw):
        return opts(**dict(dict(tail_g_u=p, tail_geo=p, tail_forces=p, tail_n_edges=E, tail_n_layers=3, tail_cutoff=5.0), **kw))

    def refused(rc, who, needle):
        assert rc == E_INVALID, (who, rc)
        msg = L.nnhip_last_error().decode()
        assert msg.startswith(who + ': bad arguments (') and needle in msg, msg
    done = C.c_int32(7)
    msg_bwd = lambda n, need_gm, o, d: L.nnhip_message_bwd_ex(p, p, p, p, p, p, p, p, p, p, n, need_gm, o, d, None)  # noqa: E731
    refused(msg_bwd(N, 0, None, None), 'nnhip_message_bwd_ex', 'opts')
    refused(msg_bwd(-1, 0, C.byref(opts()), None), 'nnhip_message_bwd_ex', 'n_atoms >= 0')
    refused(msg_bwd(N, 1, C.byref(tail()), C.byref(done)), 'nnhip_message_bwd_ex', '!need_gm')       # the force tail: layer 0 only,
    refused(msg_bwd(N, 0, C.byref(tail()), None), 'nnhip_message_bwd_ex', 'tail_done')                # with somewhere to report,
    for kw in (dict(rev=None), dict(mol_ptr=None), dict(pair_ptr=None), dict(tail_g_u=None), dict(tail_geo=None), dict(tail_cutoff=0.0),
               dict(tail_n_layers=0), dict(tail_n_layers=abi.CONSTANTS['NNHIP_MAX_LAYERS'] + 1), dict(tail_n_edges=-1), dict(n_mol=0),
               dict(n_mol=4), dict(n_mol=-1)):                                                         # everything the kernel reads,
        refused(msg_bwd(N, 0, C.byref(tail(**kw)), C.byref(done)), 'nnhip_message_bwd_ex', 'opts')    # molecules of <= 24 atoms on average
    assert done.value == 7                                   # (a refused call reports nothing)
    assert msg_bwd(0, 0, C.byref(tail(n_mol=1)), C.byref(done)) == OK and done.value == 0
    refused(L.nnhip_message_bwd_ex(p, p, p, p, p, p, p, p, None, p, N, 1, C.byref(opts()), None, None), 'nnhip_message_bwd_ex', 'g_m')
    ffwd = lambda n, o, phi2=p, f_out=p: L.nnhip_force_message_fwd_ex(p, phi2, p, p, p, p, p, p, f_out, n, o, None)  # noqa: E731
    refused(ffwd(N, None), 'nnhip_force_message_fwd_ex', 'opts')
    refused(ffwd(N, C.byref(opts(n_mol=-1))), 'nnhip_force_message_fwd_ex', 'n_mol >= 0')
    refused(ffwd(N, C.byref(opts()), phi2=None), 'nnhip_force_message_fwd_ex', 'phi2')               # f_in without phi2
    refused(ffwd(N, C.byref(opts()), f_out=None), 'nnhip_force_message_fwd_ex', 'f_out')
    assert ffwd(0, C.byref(opts())) == OK
    fbwd = lambda n, o, g_fin=p, g_u=p: L.nnhip_force_message_bwd_ex(p, p, p, p, p, p, p, p, p, p, g_u, g_fin, n, o, None)  # noqa: E731
    refused(fbwd(N, None), 'nnhip_force_message_bwd_ex', 'opts')
    refused(fbwd(N, C.byref(opts()), g_fin=None), 'nnhip_force_message_bwd_ex', 'g_fin')              # f_in without g_fin
    refused(fbwd(N, C.byref(opts()), g_u=None), 'nnhip_force_message_bwd_ex', 'g_u')
    assert fbwd(0, C.byref(opts())) == OK
    geom = lambda n, o, n_layers=3, cutoff=5.0, mol=p, rev=p, virial=None, g_d=p: L.nnhip_edge_embed_bwd_ex(  # noqa: E731
        p, p, p, p, p, p, p, p, rev, mol, n, E, 7, n_layers, cutoff, g_d, p, virial, o, None)
    refused(geom(N, None), 'nnhip_edge_embed_bwd_ex', 'opts')
    refused(geom(N, C.byref(opts()), n_layers=0), 'nnhip_edge_embed_bwd_ex', 'n_layers >= 1')
    refused(geom(N, C.byref(opts()), cutoff=0.0), 'nnhip_edge_embed_bwd_ex', 'cutoff > 0.f')
    refused(geom(N, C.byref(opts()), mol=None), 'nnhip_edge_embed_bwd_ex', 'mol_ptr')                 # small_molecules without offsets
    refused(geom(N, C.byref(opts()), rev=None), 'nnhip_edge_embed_bwd_ex', 'rev')
    refused(geom(N, C.byref(opts()), virial=p, g_d=None), 'nnhip_edge_embed_bwd_ex', 'g_d')           # the virial is formed from g_d,
    big = L.nnhip_edge_embed_bwd_ex(p, p, p, p, p, p, p, p, p, p, N, (1 << 20) + 1, 7, 3, 5.0, None, p, None, C.byref(opts()), None)
    refused(big, 'nnhip_edge_embed_bwd_ex', 'g_d')                                                     # and so are the forces of > 2^20 edges
    assert geom(0, C.byref(opts())) == OK
    head = lambda n, o, act=0, mol=p, energy=p: L.nnhip_head_out_ex(p, p, p, None, None, p, mol, n, 7, act, p, None, energy, o, None)  # noqa: E731
    refused(head(N, None), 'nnhip_head_out_ex', 'opts')
    refused(head(N, C.byref(opts()), act=99), 'nnhip_head_out_ex', 'activation')
    refused(head(N, C.byref(opts()), mol=None), 'nnhip_head_out_ex', 'mol_ptr')
    refused(head(N, C.byref(opts()), energy=None), 'nnhip_head_out_ex', 'energy')
    assert head(0, C.byref(opts())) == OK
    # the plain entry points are what they were: zero atoms is NNHIP_OK
    assert L.nnhip_message_bwd(p, p, p, p, p, p, p, p, p, p, 0, 1, None) == OK
    assert L.nnhip_head_out(p, p, p, None, None, p, p, 0, 7, 0, p, None, p, None) == OK
