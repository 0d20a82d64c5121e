"""mfrl_amd.abi without a GPU: the ctypes declarations of the mfx_* C ABI are read from include/magent_amd.h --
every declared function gets argtypes and restype, the structs are generated with the layout the hand-written classes
had, an unknown type is refused, and a bare Python int above 32 bits reaches the library whole."""
import ctypes
import types

import pytest

from test_abi_cpu import built, declared  # noqa: F401  (built: the module fixture that makes the library)

C = ctypes
VP, I, I64, U32, F, D = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_float, C.c_double


@pytest.fixture(scope="module")
def L(built):  # noqa: F811
    from mfrl_amd import lib
    return lib()


def test_every_declared_function_is_parsed():
    """declared() reads the `int` and `const char *` returns; mfx_collect_key is the header's one int64_t return."""
    from mfrl_amd import abi
    want = {n for n in declared() if n.startswith("mfx_")} | {"mfx_collect_key"}
    assert set(abi.prototypes()) == want


def test_every_exported_function_is_bound(L):
    from mfrl_amd import abi
    for name, (restype, argtypes) in abi.prototypes().items():
        fn = getattr(L, name, None)
        assert fn is not None, name                 # (test_abi_cpu: the library exports every declared symbol)
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes), name
        assert fn.restype is restype, name


MAPPING = {
    "mfx_rows_copy_shift": (I, [I, VP, VP, VP, VP, I64, I64, I64, I64, I64, U32, I64, VP]),    # int64_t, uint32_t, void *const *
    "mfx_qtrain_set_hyper": (I, [VP, D, D, D, D, D, D]),
    "mfx_qtrain_run": (I, [VP, VP, C.c_longlong, VP, I, I, VP, VP]),                            # long long, struct pointer
    "mfx_acnet_blob_size": (I, [I, I, I, I, VP, VP]),                                           # size_t *
    "mfx_qnet_set_weights": (I, [VP, VP, C.c_size_t, VP]),                                      # size_t
    "mfx_score_sizes": (I, [I, I64, VP]),                                                       # size_t bytes[5]
    "mfx_rule_act": (I, [VP, VP, VP, I, F, U32, U32, I, VP, VP]),
    "mfx_battle_rollout_buffer": (I, [VP, C.c_char_p, I, VP, VP]),                              # const char *, void **, size_t *
    "mfx_battle_rollout_init": (I, [VP, VP, VP, VP, I, F, C.c_uint, I]),                        # unsigned, const int *const *
    "mfx_collect_key": (I64, [I64] * 5),
    "mfx_last_error": (C.c_char_p, []),
}


@pytest.mark.parametrize("name", sorted(MAPPING))
def test_mapping(name):
    """Literal expected types.  No mfx_* function takes a bool; `unsigned` is mfx_battle_rollout_init's seed."""
    from mfrl_amd import abi
    restype, argtypes = abi.prototypes()[name]
    assert (restype, list(argtypes)) == MAPPING[name]


def test_bool_is_mapped():
    from mfrl_amd import abi
    protos, _ = abi.parse("int mfx_flag(void *game, bool on, const bool *flags);")
    assert protos == {"mfx_flag": (I, [VP, C.c_bool, VP])}


@pytest.mark.parametrize("text, fn, typ", [
    ("int mfx_ok(int a);\nint mfx_odd(int n, wchar_t c);", "mfx_odd", "wchar_t c"),
    ("int mfx_odd(struct thing *p);", "mfx_odd", "struct thing *p"),
    ("int mfx_odd(mfx_nowhere *p);", "mfx_odd", "mfx_nowhere *p"),
    ("int mfx_odd(float);", "mfx_odd", "float"),
    ("void *mfx_odd(int a);", "mfx_odd", "void *"),
])
def test_unknown_type_is_refused(text, fn, typ):
    from mfrl_amd import abi
    with pytest.raises(abi.HeaderError) as ex:
        abi.parse(text)
    assert fn in str(ex.value) and typ in str(ex.value)


def test_declaration_of_another_form_is_refused():
    from mfrl_amd import abi
    with pytest.raises(abi.HeaderError, match="mfx_cb"):
        abi.parse("int mfx_cb(int (*fn)(int), void *arg);")


STRUCTS = {     # the field lists of the hand-written classes these replace, and their sizes
    "mfx_collect_src": ([(k, VP) for k in ("view", "feat", "actions", "rewards", "mean", "stats", "counts", "ids", "alive")]
                        + [(k, C.c_int32) for k in ("n_envs", "n_groups", "group", "rowcap", "view_floats", "feat_floats",
                                                    "n_action", "mean_stride")], 104),
    "mfx_collect_dst": ([(k, VP) for k in ("obs", "feat", "act", "rew", "term", "prob", "key")] + [("capacity", I64)], 64),
    "mfx_score_src": ([(k, VP) for k in ("group_num", "alive", "stats", "agent_steps")]
                      + [(k, C.c_int32) for k in ("n_envs", "n_groups", "rowcap")], 48),
    "mfx_score_dst": ([(k, VP) for k in ("carry", "ret0", "totals", "log", "state")]
                      + [(k, I64) for k in ("ep_cap", "target")], 56),
    "mfx_trace_src": ([(k, VP) for k in ("group_num", "alive", "stats", "agent_steps", "actions", "ids", "rewards", "rng")]
                      + [(k, C.c_int32) for k in ("n_envs", "n_groups", "rowcap")], 80),
    "mfx_trace_dst": ([(k, VP) for k in ("envs", "carry", "head", "actions", "ids", "rewards", "alive", "state", "seeds")]
                      + [("cap_steps", I64), ("n_watch", C.c_int32)], 88),
    "mfx_qtrain_ring": ([(k, VP) for k in ("obs0", "feat0", "actions", "rewards", "terminals", "masks", "prob")], 56),
    "mfx_actrain_rows": ([(k, VP) for k in ("obs", "feat", "act", "ret", "prob")], 40),
}
ALIASES = {"mfx_collect_src": ("replay", "_CollectSrc"), "mfx_collect_dst": ("replay", "_CollectDst"),
           "mfx_score_src": ("scoreboard", "_ScoreSrc"), "mfx_score_dst": ("scoreboard", "_ScoreDst"),
           "mfx_trace_src": ("recorder", "_TraceSrc"), "mfx_trace_dst": ("recorder", "_TraceDst"),
           "mfx_qtrain_ring": ("qtrain", "_Ring"), "mfx_actrain_rows": ("actrain", "_Rows")}


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout(name):
    import importlib
    from mfrl_amd import abi
    fields, size = STRUCTS[name]
    S = abi.struct(name)
    assert S._fields_ == fields
    assert ctypes.sizeof(S) == size
    module, alias = ALIASES[name]
    assert getattr(importlib.import_module("mfrl_amd." + module), alias) is S


def test_struct_with_inline_arrays_is_refused_not_guessed():
    """mfx_score_record holds int32_t nums[2]: nothing uses it, and asking for it raises instead of mapping the array
    to a pointer (the rule of array parameters)."""
    from mfrl_amd import abi
    with pytest.raises(abi.HeaderError, match="nums"):
        abi.struct("mfx_score_record")


def test_a_bare_int_above_32_bits_arrives_whole(L):
    from mfrl_amd.replay import rollout_key
    assert L.mfx_collect_key(3, 2 ** 33 + 1, 17, 5, 136) == rollout_key(3, 2 ** 33 + 1, 17, 5, 136)


def test_a_float_for_an_int_is_refused(L):
    with pytest.raises(ctypes.ArgumentError):
        L.mfx_collect_key(3, 2.0, 17, 5, 136)
    n, off = ctypes.c_size_t(), (ctypes.c_size_t * 18)()
    with pytest.raises(ctypes.ArgumentError):
        L.mfx_qnet_blob_size(34.0, 21, 1, ctypes.byref(n), off)
    assert L.mfx_qnet_blob_size(34, 21, 1, ctypes.byref(n), off) == 0 and n.value > 0


def _stub(*names, **preset):
    fns = {k: types.SimpleNamespace(argtypes=None, restype=ctypes.c_int) for k in names}
    for k, v in preset.items():
        fns[k] = types.SimpleNamespace(argtypes=v, restype=ctypes.c_int)
    return types.SimpleNamespace(**fns)


def test_bind_skips_what_the_library_lacks():
    from mfrl_amd import abi
    stub = _stub("mfx_collect_key", "mfx_last_error")
    assert abi.bind(stub) is stub
    assert stub.mfx_collect_key.argtypes == [I64] * 5 and stub.mfx_collect_key.restype is I64
    assert stub.mfx_last_error.restype is C.c_char_p
    assert not hasattr(stub, "mfx_qnet_forward")


def test_bind_keeps_argtypes_that_are_set():
    from mfrl_amd import abi
    mine = [VP, I, I, VP, I]
    stub = abi.bind(_stub("mfx_battle_get", mfx_env_get_rows=mine))
    assert stub.mfx_env_get_rows.argtypes is mine
    assert stub.mfx_battle_get.argtypes == [VP, I, I, VP, I]
