"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every
symbol ``include/recsys_hip.h`` declares, and the ctypes mirror (``_lib.SIGNATURES``, ``RESTYPES``, the
``Structure`` classes) agrees with the header prototype by prototype and field by field (no compute calls: no
GPU here)."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "recsys_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|int64_t) (rs_\w+)\(", text, flags=re.M)))


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for required in ["rs_gemm", "rs_attn_fwd", "rs_attn_bwd", "rs_embed_fwd", "rs_embed_bwd",
                     "rs_layernorm_fwd", "rs_layernorm_bwd", "rs_sampled_logits_fwd", "rs_bce_fwd",
                     "rs_ce_fwd", "rs_adam_step", "rs_vocab_head_form"]:
        assert required in syms


def test_library_exports_every_declared_symbol():
    import rbm_amd._lib as L
    assert os.path.exists(L.LIB_PATH), "build the library first (__graft_entry__.build())"
    h = ctypes.CDLL(L.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(h, s), s
    assert set(L.SIGNATURES) == set(declared_symbols())
    assert L.lib().rs_abi_version() == 2


# ------------------------------------------------------------------ the header against the ctypes mirror
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}


def header_text():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def c_kind(decl, structs=()):
    """kind of a C parameter / field declaration: 'pointer', a scalar type name, or ('struct', name)"""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if words[0] in structs:
        return ("struct", words[0])
    assert words[0] in SCALARS, decl
    return words[0]


def ctypes_kind(t, struct_names):
    if isinstance(t, type) and issubclass(t, ctypes.Structure):
        return ("struct", struct_names[t])
    if t is ctypes.c_void_p or t is ctypes.c_char_p or hasattr(t, "contents") or issubclass(t, ctypes._Pointer):
        return "pointer"
    for name, ct in SCALARS.items():
        if t is ct:
            return name
    raise AssertionError(t)


def header_prototypes():
    """name -> (return type, [parameter kinds])"""
    out = {}
    for ret, name, params in re.findall(r"^(int|int64_t) (rs_\w+)\(([^;{}]*?)\);", header_text(), flags=re.M | re.S):
        params = " ".join(params.split())
        out[name] = (ret, [] if params in ("", "void") else [c_kind(q) for q in params.split(",")])
    return out


def header_structs():
    """name -> [(field, kind)] for every typedef'd struct, in declaration order"""
    text = header_text()
    found = re.findall(r"typedef struct(?: \w+)? \{(.*?)\}\s*(\w+);", text, flags=re.S)
    names = [n for _, n in found]
    out = {}
    for body, name in found:
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            m = re.match(r"^(.*?[\s*])(\w+(?:\s*,\s*\w+)*)$", decl)
            assert m, decl
            for f in m.group(2).split(","):
                fields.append((f.strip(), c_kind(m.group(1), names)))
        out[name] = fields
    return out


def test_every_prototype_matches_its_signature():
    """parameter count, per-parameter kind (pointer, int, int64_t, uint64_t, float, double) and return type of
    every prototype of the header against SIGNATURES / RESTYPES"""
    import rbm_amd._lib as L
    protos = header_prototypes()
    assert set(protos) == set(declared_symbols()) == set(L.SIGNATURES) and len(protos) > 100
    names = {cls: n for n, cls in L.STRUCTS.items()}
    for name, (ret, kinds) in sorted(protos.items()):
        assert [ctypes_kind(t, names) for t in L.SIGNATURES[name]] == kinds, name
        assert L.RESTYPES.get(name, ctypes.c_int) is SCALARS[ret], name
    assert set(L.RESTYPES) <= set(protos)


def test_every_mirrored_struct_matches_the_header():
    """field names, order and kinds (nested structs by type) against _fields_, and ctypes.sizeof against
    rs_abi_sizeof: with natural alignment on both sides that is the same layout"""
    import rbm_amd._lib as L
    structs = header_structs()
    assert set(structs) == set(L.STRUCTS)
    names = {cls: n for n, cls in L.STRUCTS.items()}
    index = {"rs_" + n.lower(): int(i) for n, i in re.findall(r"RS_SIZEOF_(\w+) = (\d+)", header_text())}
    assert set(index) == set(structs) and sorted(index.values()) == list(range(len(structs)))
    assert [index[n] for n in L.STRUCTS] == list(range(len(structs)))        # STRUCTS is in index order
    for name, cls in L.STRUCTS.items():
        assert [(f, ctypes_kind(t, names)) for f, t in cls._fields_] == structs[name], name
        assert ctypes.sizeof(cls) == L.lib().rs_abi_sizeof(index[name]), name
    assert L.lib().rs_abi_sizeof(len(structs)) == -1 and L.lib().rs_abi_sizeof(-1) == -1


ARG, UNSUPPORTED = 1001, 1002
# A 16-byte aligned non-NULL address that points at nothing.  Every case of the test below must be rejected by the
# entry's host-side validation: a case that validation would let through would launch with this pointer on a GPU
# machine, so add none that is valid.
FAKE = 0x10000


def _filled(cls, **set_):
    """every pointer of the struct non-NULL, every M the same, sizes a valid shape of width 64"""
    sizes = {"M": 32, "T": 16, "ldx": 64, "ldwt": 192, "ncount": 1}
    a = cls()
    for f, t in cls._fields_:
        if isinstance(t, type) and issubclass(t, ctypes.Structure):
            setattr(a, f, _filled(t))
        elif t is ctypes.c_void_p:
            setattr(a, f, FAKE)
        elif f in sizes:
            setattr(a, f, sizes[f])
    for k, v in set_.items():
        obj = a
        *path, leaf = k.split("__")
        for q in path:
            obj = getattr(obj, q)
        setattr(obj, leaf, v)
    return a


def test_row_chain_entries_reject_bad_arguments_before_any_launch():
    """M <= 0, d = 96, two structs with different M, o without delta, a head without count_parts: RS_ERR_ARG or
    RS_ERR_UNSUPPORTED from every row-chain entry that takes the argument (a call that got as far as a launch would
    return the runtime's own error, or fault)"""
    import rbm_amd._lib as L
    lib = L.lib()
    plain_in = dict(e__item_emb=None)
    entries = {     # name -> the classes of its struct arguments
        "rs_sas_block_in": (L.SasInArgs,), "rs_sas_block_out": (L.SasOutArgs,),
        "rs_sas_block_out_bwd_delta": (L.SasOutBwdArgs,), "rs_sas_block_in_bwd": (L.SasInBwdArgs,),
        "rs_sas_block_out_in": (L.SasOutArgs, L.SasInArgs),
        "rs_sas_block_in_out_bwd": (L.SasInBwdArgs, L.SasOutBwdArgs),
        "rs_sas_block_out_head_bwd": (L.SasOutArgs, L.SasOutBwdArgs)}
    assert set(entries) == {n for n, sig in L.SIGNATURES.items() if any(hasattr(t, "contents") and issubclass(
        t._type_, (L.SasInArgs, L.SasOutArgs, L.SasOutBwdArgs, L.SasInBwdArgs)) for t in sig)}

    def args(name, **set_):
        """valid arguments of the entry (out_in: no head and no embed form), then set_ applied to every struct
        that has the field"""
        out = []
        for cls in entries[name]:
            base = {}
            if name == "rs_sas_block_out_in":
                base = dict(h__E=None) if cls is L.SasOutArgs else plain_in
            own = {k: v for k, v in set_.items() if hasattr(cls, k.split("__")[0])}
            out.append(_filled(cls, **{**base, **own}))
        return out

    def code(name, d, structs):
        return getattr(lib, name)(d, *structs, None)

    for name in entries:
        for M in (0, -16):
            assert code(name, 64, args(name, M=M)) == ARG, (name, M)
        assert code(name, 96, args(name)) in (ARG, UNSUPPORTED), name
        assert code(name, 96, args(name, ldwt=288)) in (ARG, UNSUPPORTED), name
        if len(entries[name]) == 2:
            a, b = args(name)
            b.M = a.M + 16
            assert code(name, 64, [a, b]) == ARG, name
    assert code("rs_sas_block_in", 96, args("rs_sas_block_in", **plain_in)) == UNSUPPORTED
    for name in ("rs_sas_block_out_bwd_delta", "rs_sas_block_in_out_bwd"):
        assert code(name, 64, args(name, delta=None)) == ARG, name           # o without delta
        assert code(name, 64, args(name, o=None)) == ARG, name               # and the reverse
    for name in ("rs_sas_block_out", "rs_sas_block_out_head_bwd"):
        assert code(name, 64, args(name, h__count_parts=None)) == ARG, name
    assert code("rs_sas_block_out_head_bwd", 64, args("rs_sas_block_out_head_bwd", h__E=None)) == ARG   # needs a head
    assert code("rs_sas_block_out_in", 64, args("rs_sas_block_out_in", h__E=FAKE)) == ARG               # takes none
    assert code("rs_sas_block_in_bwd", 64, args("rs_sas_block_in_bwd", ldwt=128)) == ARG
    assert code("rs_sas_block_in", 64, args("rs_sas_block_in", ldx=68, **plain_in)) == ARG


def test_grouped_wgrad_slab_size_host_function():
    """rs_wgrad_grouped_slab_numel is host-only: the Python sizing helper must agree with it."""
    import rbm_amd._lib as L
    from rbm_amd import ops
    shapes = [(128, 128), (256, 128), (64, 64)]
    arr = (L.WgradProblem * 3)(*[L.WgradProblem(None, N, None, K, N, K, None, None) for N, K in shapes])
    for M, rows in [(25600, 640), (111, 64), (64, 128)]:
        assert L.lib().rs_wgrad_grouped_slab_numel(3, arr, M, rows) == ops.wgrad_grouped_slab_numel(shapes, M, rows)


def test_product_path_does_not_import_oracle():
    pkg = os.path.join(ROOT, "recommender-baseline-model_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
