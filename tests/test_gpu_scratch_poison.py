"""Library-owned scratch held to poison (HEAMD_SCRATCH_POISON, csrc/scratch_cache.cpp).

tests/test_gpu_footprint.py poisons the workspaces a CALLER hands in.  Scratch the library lends itself -- `workspace = NULL`,
and every protocol entry that owns its scratch -- is driver-cleared memory the first time and the previous call's data from
then on, and the suite repeats calls on the same inputs: a read before the write, a block handed on too early, or work on a side
lane that outlives the release computes the right words from leftovers.  With the switch on, every block is filled with the poison
byte before its caller sees it and with the complement byte when it goes back (the block cache's blocks: a captured stream's
scratch, from the HIP pool, is left alone).

Every case of tests/scratch_sites.py runs under 0xA5 and 0xFF (words above every modulus), with the block cache at its default
(it keeps no block whose release has completed) and told to keep everything:
  * the workspace-taking rows of tests/footprint_cases.py with `workspace = NULL`, at SMALL, TILED, their FORMS shapes and at
    N = 256 (the ring of tests/c/abi_scheme.c, which no footprint shape has): the six pipelines of ORACLE_ROWS equal the CPU
    oracle word for word, the others the words of the same call without the switch;
  * the protocol, client, database and keyword entries through a test of their own file at its smallest shape -- each of those
    compares with its reference itself.
With the cache on, after trim_scratch(0) and the call, scratch_cached_bytes() > 0: the case really took library scratch."""
import contextlib

import numpy as np
import pytest

import aliasing_cases as A
import footprint
import footprint_cases as F
import heamd
import scratch_sites

pytestmark = pytest.mark.gpu

OK = 0
POISONS = (0xA5, 0xFF)
SOURCES = ("default", "cache")  # he_set_scratch_cache(0): keep nothing that has completed; (): keep everything
N256 = F.shape("N256", 256, {64: (50, 50, 51), 32: (27, 28, 28)}, "the ring of tests/c/abi_scheme.c: log_degree < 12, the unfused "
               "forms on more than one workgroup", batch=3, L=2)


@contextlib.contextmanager
def library_scratch(monkeypatch, source, poison, takes_scratch=True):
    """The switch and the cache's limit for the calls inside; the default limit (0) and no switch afterwards"""
    with monkeypatch.context() as patch:
        if poison is None:
            patch.delenv("HEAMD_SCRATCH_POISON", raising=False)
        else:
            patch.setenv("HEAMD_SCRATCH_POISON", str(poison))
        try:
            if source == "cache":
                heamd.set_scratch_cache()
                heamd.trim_scratch(0)
            yield
            import torch

            torch.cuda.synchronize()
            if source == "cache" and takes_scratch:
                assert heamd.scratch_cached_bytes() > 0, "the case took no library scratch"
        finally:
            heamd.set_scratch_cache(0)


# ---- the workspace pipelines with workspace = NULL ---------------------------------------------------------------------------
ROWS = [row for row in A.CASES if row.name in F.WORKSPACE]
BFV_CASES = [(row, w, shp) for row in ROWS for shp in F.shapes(row) + [N256] for w in F.words_of(row, shp)]
BFV_IDS = ["%s-u%d-%s" % (row.name, 8 * w, shp.name) for row, w, shp in BFV_CASES]


@pytest.mark.parametrize("row,word_bytes,shp", BFV_CASES, ids=BFV_IDS)
def test_workspace_pipelines_on_library_scratch(oracle, monkeypatch, row, word_bytes, shp):
    import torch

    from test_gpu_footprint import as_bytes, contexts, host_fill, oracle_outputs

    lib = heamd.load_library()
    degree = F.degree_of(row, shp)
    ours, ref, moduli = contexts(oracle, row.context, word_bytes, degree, shp.bits[8 * word_bytes])
    name = row.name + "_u32" if (row.words == "twin" and word_bytes == 4) else row.name
    for variable, value in shp.setenv.items():
        monkeypatch.setenv(variable, value)
    env = F.environment(row, shp, moduli, word_bytes)
    env["workspace_bytes"] = 32  # the slab is laid out and never handed in
    sizes = A.slab_bytes(row, env)
    arena = footprint.layout(sizes, row.written)
    kinds = F.FILLS[row.name]
    spans = {slab: footprint.span(arena, slab) for slab in row.slabs}
    if shp.alias is not None:
        written_alias, read_alias = shp.alias
        spans[written_alias] = (arena.offsets[read_alias], arena.offsets[read_alias] + sizes[written_alias])
    rng = np.random.default_rng(len(BFV_IDS) + sum(map(ord, name + shp.name)))
    qbsk = ours.qbsk_context(env["L"]).moduli if "qbsk" in kinds.values() else None
    host = {slab: host_fill(kind, rng, sizes[slab], env, moduli, qbsk, ours.t) for slab, kind in kinds.items()
            if kind not in F.POISONED}
    device = {slab: torch.from_numpy(as_bytes(array, kinds[slab], word_bytes).copy()).cuda() for slab, array in host.items()}
    backing = torch.empty(arena.total + footprint.ALIGN, dtype=torch.uint8, device="cuda")
    skew = -backing.data_ptr() % footprint.ALIGN
    memory = backing[skew: skew + arena.total]
    where = {slab: memory.data_ptr() + begin for slab, (begin, _) in spans.items()}
    where["workspace"] = None
    results = [slab for slab in row.written if slab != "workspace"]

    def call(what):
        memory.fill_(footprint.GUARD_BYTE)
        for slab, kind in kinds.items():
            begin, end = footprint.span(arena, slab)
            if kind in F.POISONED:
                memory[begin:end] = 0x3C
            else:
                memory[begin:end] = device[slab]
        status, text = A.invoke(lib, row, name, ours.h, dict(env, workspace_bytes=0), where)
        torch.cuda.synchronize()
        assert status == OK, (name, shp.name, what, status, text)
        return {slab: memory[slice(*spans[slab])].clone() for slab in results}

    # csrc/bfv_api.cpp secret_dot_product: `is_eval` transforms nothing and `!is_eval && poly_count == 1` is c0 itself -- neither
    # copies into scratch, and decrypt_dot then asks for none
    takes_scratch = not (row.name == "he_bfv_secret_dot_product_device" and (env["is_eval"] or env["polys"] == 1))
    with library_scratch(monkeypatch, "default", None):
        plain = call("no switch")
    expected = plain
    if row.name in F.ORACLE_ROWS:
        word = np.uint32 if word_bytes == 4 else np.uint64
        expected = {slab: torch.from_numpy(np.ascontiguousarray(np.asarray(words).reshape(-1).astype(word)).view(np.uint8)).cuda()
                    for slab, words in oracle_outputs(row, ref, env, host).items()}
    for source in SOURCES:
        for poison in POISONS:
            what = "scratch from the %s over 0x%02X" % (source, poison)
            with library_scratch(monkeypatch, source, poison, takes_scratch):
                got = call(what)
            for slab in results:
                wrong = int((got[slab] != expected[slab]).sum().item())
                assert wrong == 0, "%s %s, %s: %d bytes of %s differ" % (name, shp.name, what, wrong, slab)


# ---- the entries that own their scratch: a test of their own file, under the switch --------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("poison", POISONS, ids=["0xA5", "0xFF"])
@pytest.mark.parametrize("name", sorted(scratch_sites.DELEGATED))
def test_entries_that_own_their_scratch(request, monkeypatch, name, poison, source):
    case = scratch_sites.DELEGATED[name]
    # the entries tests/scratch_sites.py says this case calls: each one has to be called, through the binding's own library object
    lib, called = heamd.load_library(), set()
    for entry in sorted({s.entry for s in scratch_sites.SITES if s.case == name}):
        def counted(*args, _entry=entry, _original=getattr(lib, entry)):
            called.add(_entry)
            return _original(*args)

        monkeypatch.setattr(lib, entry, counted)
    with library_scratch(monkeypatch, source, poison):
        function, arguments = scratch_sites.resolve(case, request)
        function(**arguments)
    missed = sorted({s.entry for s in scratch_sites.SITES if s.case == name} - called)
    assert not missed, "%s never called %s" % (name, missed)
