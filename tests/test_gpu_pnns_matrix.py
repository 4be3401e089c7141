"""The PNNS server response to query matrices of several rows on the device (he_pnns_mul_transpose_matrix_device /
he_pnns_compute_response_matrix_device and their UInt32 twins) against tests/pnns_matrix_reference.py's restatement of
mulTranspose(matrix:) over the CPU oracle, plus the oracle's modSwitchDown chain: word for word.  Word equality needs no valid
encryption, so queries and Galois keys are uniform canonical words, distinct per client; the decryption test uses real ones.
Each shape of TABLE is the smallest that reaches the branch named next to it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import heamd
import pnns_matrix_reference as pm
import pnns_reference as pnns
from bfv_helpers import BfvClient
from test_gpu_pnns import parameters
from test_gpu_pnns_response import get_setup, to_device, uniform_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, L, rows, cols, R, Q)
TABLE = [
    (64, 3, 10, 4, 3, 1),      # one (last) query ciphertext, copies > 1, rotateCount > 0, one half-chunk, no swap in packing
    (64, 3, 10, 4, 5, 2),      # chunk of 3 + 2: swapRowsAndAdd; two clients
    (64, 3, 10, 4, 7, 1),      # two result ciphertexts, the second a ragged chunk of one
    (64, 3, 10, 4, 20, 1),     # two query ciphertexts: a non-last one (copies = 1, rotateCount = 7), the early-stopping scan,
                               # rows with different rotateCount in one batch
    (64, 3, 10, 32, 3, 1),     # P = N / 2: rotateCount = 0, slot [3] NULL and not read
    (64, 3, 32, 4, 3, 1),      # cps = 1: swap only, the pack plan is not read (empty plan, no pack keys)
    (64, 3, 70, 4, 3, 1),      # cps = 0, C = 2: no packing, R C results
    (64, 3, 10, 4, 1, 3),      # R = 1: the existing entry's words; slots [2], [3] and the pack keys all NULL
    (256, 2, 20, 100, 2, 1),   # L = 2, P = N / 2, ragged last giant step
    (1024, 3, 100, 16, 5, 2),  # the tile kernel, ten vectors in passes of 4 + 4 + 2 across a client boundary
    (4096, 4, 100, 16, 3, 1),  # L = 4
]
PLANS_OF_TEN = [[(10, 1)], [(8, 1), (2, 1)], [(2, 1), (8, 1)]]


def element_of_for(degree):
    def element_of(step):
        if step == "swap":
            return heamd.galois_element_swapping_rows(degree)
        return heamd.galois_element_rotating_columns(step, degree)

    return element_of


def setup_for(oracle, degree, L, word32=False):
    s = get_setup(oracle, degree, word32=word32, two_moduli=(L == 2))
    assert s.ref.L == L
    return s


class Case:
    """Inputs of one call: the matrix, Q clients' queries and keys (a key per Galois element, so two slots of one element hold
    the same words, as a real evaluation key does).  shared: {client: the client whose keys it is handed, words and device
    tensors alike}."""

    def __init__(self, s, rows, cols, row_count, clients, plan, seed, baby_step=None, shared=None):
        import torch

        self.s, self.rows, self.cols, self.row_count, self.clients, self.plan = s, rows, cols, row_count, clients, list(plan)
        rng = np.random.default_rng(seed)
        n, L = s.degree, s.ref.L
        self.baby_step = baby_step or pnns.baby_step_giant_step(cols)[0]
        self.needs = pm.needs(n, rows, cols, row_count, self.baby_step)
        values = rng.integers(-(s.t >> 1), ((s.t - 1) >> 1) + 1, size=(rows, cols), dtype=np.int64)
        self.matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(values).cuda(), baby_step=self.baby_step)
        assert int(flag.item()) == 0
        self.query_ciphertexts = pnns.plaintext_count(n, row_count, cols, "denseRow")
        q_moduli, ks_moduli = list(s.q[:L]), list(s.q[:L]) + [s.q[-1]]
        self.query = uniform_words(rng, q_moduli, (clients, self.query_ciphertexts, 2), n)
        element_of = element_of_for(n)
        self.slot_steps = [-1, -self.baby_step, "swap", pnns.next_power_of_two(cols)] + [step for step, _ in self.plan]
        self.slot_needed = [0 in self.needs, 1 in self.needs, 2 in self.needs, 3 in self.needs] + \
            ["pack" in self.needs] * len(self.plan)
        elements = sorted({element_of(step) for step, needed in zip(self.slot_steps, self.slot_needed) if needed})
        # per client: element -> words, drawn in the order of the elements, so a plan's order does not change a key
        self.keys = [{element: uniform_words(rng, ks_moduli, (L, 2), n) for element in elements} for _ in range(clients)]
        for client, other in (shared or {}).items():
            self.keys[client] = self.keys[other]

    def device_keys(self, drop=None):
        """Per client the list of 4 + len(plan) device tensors, None where the shape does not need the slot (or slot `drop`)."""
        element_of = element_of_for(self.s.degree)
        rows = {}  # one row of tensors per distinct key set
        for by_element in self.keys:
            if id(by_element) in rows:
                continue
            cache = {element: to_device(self.s, words) for element, words in by_element.items()}
            rows[id(by_element)] = [cache[element_of(step)] if needed and slot != drop else None
                                    for slot, (step, needed) in enumerate(zip(self.slot_steps, self.slot_needed))]
        return [rows[id(by_element)] for by_element in self.keys]

    def expected(self):
        """-> (mulTranspose [Q][M][2][L][N], response [Q][M][2][1][N])"""
        s = self.s
        matrix_host = s.to_host(self.matrix)
        full, single = [], []
        for q in range(self.clients):
            result = pm.mul_transpose_matrix(s.ref, s.encoder, element_of_for(s.degree), matrix_host, self.rows, self.cols,
                                             self.baby_step, self.query[q], self.row_count, self.plan,
                                             pm.Keys(s.ref, self.keys[q]))
            full.append(result)
            down = result
            for level in range(s.ref.L, 1, -1):
                down = s.ref.mod_switch_down(down, 2, level)
            single.append(down)
        return np.stack(full), np.stack(single)

    def run(self, entry="mul_transpose_matrix", keys=None, stream=None, query=None):
        s = self.s
        query = to_device(s, self.query) if query is None else query
        return getattr(s.pnns, entry)(self.matrix, self.rows, self.cols, query, self.row_count, self.plan,
                                      self.device_keys() if keys is None else keys, baby_step=self.baby_step, stream=stream)


def default_plan(degree, rows, cols, row_count):
    return [(rows, 1)] if "pack" in pm.needs(degree, rows, cols, row_count) else []


def check(case):
    s = case.s
    full, single = case.expected()
    got_full = s.to_host(case.run("mul_transpose_matrix"))
    got_single = s.to_host(case.run("compute_response_matrix"))
    label = (s.degree, s.word32, case.rows, case.cols, case.row_count, case.clients, case.plan)
    count = pm.result_ciphertext_count(s.degree, case.rows, case.row_count)
    assert full.shape == (case.clients, count, 2, s.ref.L, s.degree), label
    assert got_full.shape == full.shape and got_single.shape == single.shape, label
    assert full.any() and single.any(), label
    assert np.array_equal(got_full, full), label
    assert np.array_equal(got_single, single), label
    return full


@pytest.mark.parametrize("degree,L,rows,cols,row_count,clients", TABLE)
def test_words_of_the_table(oracle, degree, L, rows, cols, row_count, clients):
    s = setup_for(oracle, degree, L)
    case = Case(s, rows, cols, row_count, clients, default_plan(degree, rows, cols, row_count), 100 * degree + rows + row_count)
    shape = s.pnns.query_matrix_shape(rows, cols, row_count)
    assert shape["needs"] == case.needs == pm.needs(degree, rows, cols, row_count)
    assert shape["query_ciphertexts"] == case.query_ciphertexts
    full = check(case)
    if row_count == 1:  # the existing entry's words; keys [2], [3] and the plan's are NULL
        assert case.needs == {0, 1} and case.plan == []
        one_row = s.pnns.mul_transpose(case.matrix, rows, cols, to_device(s, case.query[:, 0]),
                                       [(keys[0], keys[1]) for keys in case.device_keys()], baby_step=case.baby_step)
        assert np.array_equal(s.to_host(one_row), full)


@pytest.mark.parametrize("row_count,clients", [(3, 1), (5, 2), (7, 1), (20, 1)])
def test_pack_plans_in_the_given_order(oracle, row_count, clients):
    """rows = 10 at N = 64 with the plans {10}, {8, 2} and {2, 8}: the words follow the order given."""
    s = setup_for(oracle, 64, 3)
    results = []
    for plan in PLANS_OF_TEN[1:]:  # {10} is the table's run
        results.append(check(Case(s, 10, 4, row_count, clients, plan, 7 + row_count)))
    # the same seed gives the same key words to steps 8 and 2 in either order: only the order of application differs
    assert not np.array_equal(results[0], results[1])


def test_pack_plan_with_a_repeated_step(oracle):
    s = setup_for(oracle, 64, 3)
    check(Case(s, 3, 4, 5, 1, [(1, 3)], 13))


def test_pack_plan_errors(oracle):
    s = setup_for(oracle, 64, 3)
    case = Case(s, 10, 4, 3, 1, [(10, 1)], 5)
    rows = case.device_keys()
    # not 10 mod 32; a step outside [1, 31]; no plan where the packing rotates
    for plan in ([(9, 1)], [(8, 1), (3, 1)], [(32, 1), (10, 1)], [(0, 1), (10, 1)], [(-22, 1)], []):
        case.plan = plan
        with pytest.raises(heamd.HeError) as err:
            case.run(keys=[row[:4] + [row[4]] * len(plan) for row in rows])
        assert err.value.name == "invalidArgument", plan
    check(Case(s, 10, 4, 3, 1, [(21, 2)], 5))  # 42 = 10 mod 32


@pytest.mark.parametrize("index", [1, 3, 9])
def test_words_u32(oracle, index):
    degree, _, rows, cols, row_count, clients = TABLE[index]
    s = get_setup(oracle, degree, word32=True)
    check(Case(s, rows, cols, row_count, clients, default_plan(degree, rows, cols, row_count), 32 * degree + row_count))


@pytest.mark.parametrize("word32", [False, True])
def test_two_clients_share_keys_next_to_a_third(oracle, word32):
    """TABLE[1] (R = 5: all five slots) with a third client, clients 0 and 1 handed the same device key tensors in every slot and client
    2 its own: in each Galois batch a run of two equal keys lies next to a run of one.  Queries are distinct per client, the
    expected words come per client from the restatement with that client's keys."""
    s = get_setup(oracle, 64, word32=word32)
    assert s.ref.L == 3
    case = Case(s, 10, 4, 5, 3, [(10, 1)], 64 * 5 + 3, shared={1: 0})
    keys = case.device_keys()
    for slot, needed in enumerate(case.slot_needed):
        assert needed and keys[0][slot] is keys[1][slot]
        assert keys[2][slot].data_ptr() != keys[0][slot].data_ptr()
    assert not np.array_equal(case.query[0], case.query[1])
    check(case)


def test_missing_keys_leave_out_untouched(oracle):
    """A NULL in a slot the shape needs: missingGaloisKey before anything is enqueued.  Slots 0-3 and the plan's key at
    64 / 10 x 4 / R = 5, where all five are needed."""
    import torch

    s = setup_for(oracle, 64, 3)
    case = Case(s, 10, 4, 5, 2, [(10, 1)], 21)
    assert case.needs == {0, 1, 2, 3, "pack"}
    lib = heamd.load_library()
    out = torch.full((2, 1, 2, s.ref.L, 64), 0x5A5A, dtype=torch.int64, device="cuda")
    query = to_device(s, case.query)
    plan = (heamd.binding.PnnsPackStep * 1)()
    plan[0].step, plan[0].count = 10, 1
    for slot in range(5):
        with pytest.raises(heamd.HeError) as err:
            case.run(keys=case.device_keys(drop=slot))
        assert err.value.name == "missingGaloisKey", slot
        rows = case.device_keys(drop=slot)
        keys = (heamd.binding.vp * 10)(*[None if key is None else key.data_ptr() for row in rows for key in row])
        status = lib.he_pnns_mul_transpose_matrix_device(s.pnns.h, heamd.binding.vp(case.matrix.data_ptr()), case.matrix.shape[0],
                                                         10, 4, case.baby_step, heamd.binding.vp(query.data_ptr()), 5, 2, plan, 1,
                                                         keys, heamd.binding.vp(out.data_ptr()), None)
        assert heamd.binding.STATUS_NAMES[status] == "missingGaloisKey", slot
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A).all()), slot
    # keys the shape does not need may be NULL: the table's P = N / 2, cps = 1, cps = 0 and R = 1 rows pass None there


# ---- decryption -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,rows,cols,row_count,clients", [(64, 10, 4, 5, 2), (1024, 100, 16, 5, 2)])
def test_decrypted_response_is_the_matrix_product(oracle, degree, rows, cols, row_count, clients):
    import torch

    s = setup_for(oracle, degree, 3)
    t = s.t
    rng = np.random.default_rng(degree + rows)
    bound = int(np.sqrt((t // 2 - 1) // cols))
    data = rng.integers(-bound, bound + 1, size=(rows, cols))
    baby_step, _ = pnns.baby_step_giant_step(cols)
    matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(data.astype(np.int64)).cuda())
    assert int(flag.item()) == 0
    element_of = element_of_for(degree)
    steps = [-1, -baby_step, "swap", pnns.next_power_of_two(cols), rows]
    parties = [BfvClient(oracle, s.ref, seed=degree + k) for k in range(clients)]
    vectors = [rng.integers(-bound, bound + 1, size=(row_count, cols)) for _ in parties]
    queries, keys = [], []
    for client, rows_of_client in zip(parties, vectors):
        slots = pm.dense_row_slots(np.mod(rows_of_client, t), row_count, cols, degree)
        queries.append(np.stack([client.encrypt([int(v) for v in c]) for c in s.encoder.encode(slots)]))
        keys.append([heamd.to_device(client.galois_key(element_of(step))) for step in steps])
    device_query = heamd.to_device(np.stack(queries))
    full = heamd.to_host(s.pnns.mul_transpose_matrix(matrix, rows, cols, device_query, row_count, [(rows, 1)], keys))
    single = heamd.to_host(s.pnns.compute_response_matrix(matrix, rows, cols, device_query, row_count, [(rows, 1)], keys))
    for k, (client, rows_of_client) in enumerate(zip(parties, vectors)):
        product = np.mod(data @ rows_of_client.T, t).astype(np.uint64)
        for result, moduli_count in ((full[k], None), (single[k], 1)):
            decoded = s.encoder.decode(np.array([client.decrypt(ct, moduli_count) for ct in result], dtype=np.uint64))
            assert np.array_equal(pm.unpack_dense_column(decoded, rows, row_count, degree), product), (k, moduli_count)


# ---- composition ----------------------------------------------------------------------------------------------------------------
def test_entry_equals_the_composition_of_existing_entry_points(oracle):
    """1024 / 100 x 16 / R = 5, two clients: forward NTT, he_bfv_mul_plain_device with the restatement's masks, Galois calls,
    he_pnns_mul_transpose_device over the rows, additions -- the new kernels against the library itself."""
    import torch

    degree, rows, cols, row_count, clients = 1024, 100, 16, 5, 2
    s = setup_for(oracle, degree, 3)
    case = Case(s, rows, cols, row_count, clients, [(rows, 1)], 99)
    bfv, L = s.bfv, s.bfv.L
    ring = bfv.ciphertext_context()
    element_of = element_of_for(degree)
    padded = pnns.next_power_of_two(cols)
    rows_per_ciphertext = (degree // 2 // padded) * 2
    columns_per_simd_row = (degree // 2) // rows
    got = heamd.to_host(case.run())
    device_keys = case.device_keys()
    device_query = to_device(s, case.query)

    def rotate(ct, key, step):
        return bfv.apply_galois(ct.reshape(1, 2, L, degree), element_of(step), key).reshape(2, L, degree)

    for q in range(clients):
        key_one, key_baby, key_swap, key_columns, key_pack = device_keys[q]
        extracted = []
        for r in range(row_count):
            mask, copies = pm.mask_list(r, row_count, cols, degree)
            plaintext = bfv.plaintext_to_eval(heamd.to_device(s.encoder.encode(np.array(mask, dtype=np.uint64))))
            ct = ring.forward_ntt_(device_query[q, r // rows_per_ciphertext].clone())
            ct = ring.inverse_ntt_(bfv.mul_plain_(ct, plaintext, 2))
            copy = ct
            for _ in range(pm.rotate_count(copies, cols, degree)):
                copy = rotate(copy, key_columns, padded)
                ct = ring.add_(ct.clone(), copy)
            extracted.append(ring.add_(ct.clone(), rotate(ct, key_swap, "swap")))
        products = s.pnns.mul_transpose(case.matrix, rows, cols, torch.stack(extracted).contiguous(),
                                        [(key_one, key_baby)] * row_count, baby_step=case.baby_step)
        products = [products[r, 0] for r in range(row_count)]
        packed = []
        for start in range(0, row_count, 2 * columns_per_simd_row):
            chunk = products[start:start + 2 * columns_per_simd_row]
            sums = []
            for i in range(0, len(chunk), columns_per_simd_row):
                half = list(chunk[i:i + columns_per_simd_row])
                accumulator = half.pop()
                for ct in reversed(half):
                    accumulator = ring.add_(rotate(accumulator, key_pack, rows), ct)
                sums.append(accumulator)
            packed.append(ring.add_(rotate(sums[1], key_swap, "swap"), sums[0]) if len(sums) > 1 else sums[0])
        assert len(packed) == got.shape[1]
        for m, ct in enumerate(packed):
            assert np.array_equal(heamd.to_host(ct), got[q, m]), (q, m)


# ---- groups and stream order ------------------------------------------------------------------------------------------------------
_GROUP_SCRIPT = r"""
import sys
import numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}]
import heamd
degree, t, q = {degree}, {t}, {q}
bfv = heamd.BfvContext(degree, t, q)
ctx = heamd.PnnsContext(bfv)
rng = np.random.default_rng(11)
L = bfv.L
def words(moduli, before):
    return np.stack([rng.integers(0, m, size=before + (degree,), dtype=np.uint64) for m in moduli], axis=len(before))
rows, cols, row_count = 70, 4, 3
values = rng.integers(-(t >> 1), ((t - 1) >> 1) + 1, size=(rows, cols), dtype=np.int64)
matrix, _ = ctx.diagonal_matrix(torch.from_numpy(values).cuda())
query = heamd.to_device(words(q[:L], (1, 1, 2)))
keys = [[heamd.to_device(words(q[:L] + q[-1:], (L, 2))) for _ in range(4)]]
np.savez(sys.argv[1], full=ctx.mul_transpose_matrix(matrix, rows, cols, query, row_count, [], keys).cpu().numpy(),
         single=ctx.compute_response_matrix(matrix, rows, cols, query, row_count, [], keys).cpu().numpy())
"""


def test_result_groups_give_identical_words(oracle, tmp_path):
    """HEAMD_PNNS_RESPONSE_GROUP = 1 on the cps = 0 shape (C = 2) gives the words of one group (a fresh process each: the
    override is read from the environment)."""
    degree = 64
    t, q = parameters(oracle, degree)
    script = tmp_path / "groups.py"
    script.write_text(_GROUP_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "swift-homomorphic-encryption_amd"),
                                           degree=degree, t=t, q=list(q)))
    results = []
    for group in (None, "1"):
        env = dict(os.environ)
        env.pop("HEAMD_PNNS_RESPONSE_GROUP", None)
        if group:
            env["HEAMD_PNNS_RESPONSE_GROUP"] = group
        path = tmp_path / f"out_{group}.npz"
        subprocess.run([sys.executable, str(script), str(path)], check=True, env=env, timeout=300)
        results.append(np.load(path))
    for name in ("full", "single"):
        assert results[0][name].any() and results[0][name].shape[1] == 6
        assert np.array_equal(results[0][name], results[1][name]), name


def test_back_to_back_calls_on_one_stream(oracle):
    """Two calls with different R enqueued on one stream with no host synchronisation between them (they share the
    stream-ordered scratch) give the words of the same calls each followed by a synchronisation."""
    import torch

    s = setup_for(oracle, 1024, 3)
    cases = [Case(s, 100, 16, 5, 2, [(100, 1)], 41), Case(s, 100, 16, 3, 1, [(100, 1)], 42)]
    inputs = [(to_device(s, case.query), case.device_keys()) for case in cases]
    torch.cuda.synchronize()
    apart = []
    for case, (query, keys) in zip(cases, inputs):
        apart.append(heamd.to_host(case.run("compute_response_matrix", keys=keys, query=query)))
        torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    together = [case.run("compute_response_matrix", keys=keys, query=query, stream=stream)
                for case, (query, keys) in zip(cases, inputs)]
    stream.synchronize()
    for a, b in zip(apart, together):
        assert a.any() and np.array_equal(a, heamd.to_host(b))
