// ntt_sources.hpp -- where a transform's rows come from when not from the slab itself: the constants that name each source
// and the descriptors the kernels take as their last argument.  Read by the kernel families (ntt_forward_tiled.hpp,
// ntt_inverse_tiled.hpp, ntt_interleaved.hpp), the launch policy (ntt_policy.hpp) and the routing layer (ntt_routing.hip).
// An empty descriptor is spelled {}.
#pragma once

#include <cstddef>
#include <cstdint>

namespace heamd {
namespace ntt {

// Row sources of the forward transform other than the slab itself: the step that would otherwise write the slab (and
// this kernel read it back) is applied to the words as they are loaded.
//   kSourceSpread  the key-switching decomposition (Bfv+Keys.swift:165-179): output row (poly, j, r) of a
//                  [polys][L][L+1][N] slab is the transform mod ks_modulus[r] of row j of polynomial `poly`, read
//                  straight from the ciphertext and reduced mod r first when q_j > modulus r; with galois_inverse
//                  set, of row j of the polynomial's image under the automorphism (Bfv.applyGalois key-switches
//                  galois(c1), Bfv.swift:190-196): the row is read in order and permuted through the LDS tile;
//   kSourceLift    Plaintext.convertToEvalFormat (Plaintext.swift:149-170): output row (poly, r) of a [polys][L][N]
//                  slab is the transform mod q_r of the centred lift of plaintext `poly` ([N] values < t):
//                  x < (t + 1) / 2 ? x : x + (q_r - t).
//   kSourceRows    the Q band of BEHZ's [Q, Bsk] records (Bfv+Multiply.swift:51-57): liftQToQBsk leaves rows [0, L) of
//                  a lifted polynomial equal to the input (RnsTool.swift:329-330), so row (record, r) of the band is
//                  the transform of row r of the record's source polynomial, read where the ciphertext lies instead
//                  of from a copy the lift would write: record = item * 4 + slot takes polynomial slot & 1 of item
//                  `item` of `base` (slots 0, 1) or `second` (slots 2, 3), items `stride` words apart; without a
//                  second operand, record r takes the polynomial at base + r * stride.
constexpr int kSourceSlab = 0, kSourceSpread = 1, kSourceLift = 2, kSourceRows = 3;
struct SpreadSource {
    const uint64_t* base = nullptr;  // row j of polynomial `poly` at base + poly * stride + j * N
    size_t stride = 0;
    uint32_t L = 0;        // source rows per polynomial (1 for a plaintext)
    uint64_t plaintext_modulus = 0;
    // kSourceSpread only: g^-1 mod 2N when the source polynomial is to be taken through f(x) -> f(x^g) first
    // (PolyRq/Galois.swift:115-143), 0 otherwise
    uint32_t galois_inverse = 0;
    const uint64_t* second = nullptr;  // kSourceRows only: the operand of slots 2, 3 (nullptr: one operand, consecutive polynomials)
};
// (kernel arguments are copied byte for byte: the default member initialisers must not move a field)
static_assert(sizeof(SpreadSource) == 48 && offsetof(SpreadSource, second) == 40, "SpreadSource's layout is part of the kernels' ABI");

// TENSOR: the BEHZ tensor product (Bfv+Multiply.swift:80-82) fused into the load.  The launch covers records
// (item, c), c in {0, 1, 2}, of `record_rows` rows; the words of row r of record (item, c) are computed from the four
// Eval polynomials (a0, a1, b0, b1) of the item at tensor_source + (item * 4 + k) * record_rows * N + r * N as
// a0 b0 | a0 b1 + a1 b0 | a1 b1 while they are loaded, instead of by a kernel that writes them for this one to read.
// KEYMAC: the lazy inner product with the key-switching key (Bfv+Keys.swift:180-202) fused into the load.  Records
// are (polynomial, c), c in {0, 1}, of record_rows = L + 1 rows; word k of row r is
// sum_j spread[poly][j][r][k] * key[j][c][key_row(r)][k] mod ks_modulus[r], accumulated in the carry-counting form.
// kInverseFromSlabScaled: a plain slab whose context carries t N^-1 (dropExtendedBase without the fused tensor load)
// kInverseFromKeyMacFinish: the same load, restricted to the band rows r < L, with the last step of the key switch --
// drop the special modulus (divideAndRoundQLast by the centred representative of the q_ks word, Bfv+Keys.swift:203-207)
// and add the update to the ciphertext (Bfv.swift:216-217) -- applied to the transform's canonical words before they are
// stored: the q_ks row of every (polynomial, c) comes from an earlier launch of the plain kInverseFromKeyMac kernel over
// that one band row, the rows r < L of the product are never written, and the separate finish kernel (26 row moves per
// ciphertext) is gone.
constexpr int kInverseFromSlab = 0, kInverseFromTensor = 1, kInverseFromKeyMac = 2, kInverseFromSlabScaled = 3,
              kInverseFromKeyMacFinish = 4;
constexpr bool is_key_mac(int source) { return source == kInverseFromKeyMac || source == kInverseFromKeyMacFinish; }

struct InverseSource {
    const uint64_t* first = nullptr;   // tensor: the lifted polynomials; key MAC: the spread slab
    const uint64_t* second = nullptr;  // key MAC: the key
    uint32_t L = 0, top_rows = 0;  // key MAC: source moduli, rows per key polynomial
    // kInverseFromKeyMacFinish: the ciphertexts the update is added to ([item] ct_stride words apart, polynomial c at
    // c L N; the first `added_polys` polynomials are added, the others replaced), and where the result goes
    // ([item][2][L][N]); the slab argument of the kernel is the product slab whose q_ks rows are read
    const uint64_t* ct_base = nullptr;
    size_t ct_stride = 0;
    uint64_t* out = nullptr;
    uint32_t added_polys = 0;
    // ... the Galois key switch's end (Bfv.swift:190-196): galois_inverse = g^-1 mod 2N != 0: `ct_base` holds the
    // ciphertexts BEFORE the automorphism, polynomial 0 of the result is galois(c0) + update0 -- coefficient k takes source
    // coefficient k g^-1 mod 2N, negated past N (PolyRq/Galois.swift:115-143) -- and polynomial 1 is update1;
    // expand_shift != 0 on top of that: one step of PirUtil.expand (PirUtil.swift:204-236), out = the children
    // own + c' and (own - c') x^expand_shift of every polynomial (rns_kernels.hpp ExpandTargets says where they go; own_base:
    // the ciphertexts the children are formed with).  poly_base: the launch's first polynomial in ct_base / own_base / out
    // (the spread and product slabs of a run of equal keys are passed from their own start).
    uint32_t galois_inverse = 0, expand_shift = 0;
    const uint64_t* own_base = nullptr;
    const uint32_t* targets_table = nullptr;
    size_t targets_group_size = 0, targets_group_stride = 0;
    size_t poly_base = 0;
};
static_assert(sizeof(InverseSource) == 104 && offsetof(InverseSource, poly_base) == 96,
              "InverseSource's layout is part of the kernels' ABI");

}  // namespace ntt
}  // namespace heamd
