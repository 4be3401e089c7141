"""The plan of he_simple_pir_compute_response_batch_device restated in Python (csrc/simple_pir_batch_plan.hpp): which path
a shape takes, its limbs, its pass width and the fold bound with the HEAMD_SIMPLE_PIR_FOLD_COLUMNS override -- so that a test
can assert the path it means to exercise.  A helper, not a test."""
import os

LIMB_BITS = 7
K_STEP = 64            # columns of one v_mfma_i32_16x16x64_i8
BLOCK_ROWS = 128       # database rows of one workgroup
REQUEST_TILE = 16
LIMB_PRODUCT = 127 * 127
INT32_MAX = 2**31 - 1


def tile_columns(word_bits, database_limbs):
    """columns of the request slice one workgroup stages in LDS at a time"""
    return K_STEP * ((4 if word_bits == 32 else 2) // database_limbs)


def database_limbs(plaintext_bits):
    if plaintext_bits <= 7:
        return 1
    return 2 if 9 <= plaintext_bits <= 14 else 0


def natural_fold_columns(limbs):
    return INT32_MAX // (LIMB_PRODUCT * limbs) // K_STEP * K_STEP


def fold_columns(limbs, environ=None):
    columns = natural_fold_columns(limbs)
    forced = (os.environ if environ is None else environ).get("HEAMD_SIMPLE_PIR_FOLD_COLUMNS")
    if forced and forced.isdigit() and 0 < int(forced) < columns:
        columns = max(K_STEP, int(forced) // K_STEP * K_STEP)
    return columns


def plan(plaintext_bits, ciphertext_bits, word_bits, environ=None):
    limbs = database_limbs(plaintext_bits)
    classes = -(-ciphertext_bits // LIMB_BITS)
    if limbs == 0:
        return dict(matrix_path=0, database_limbs=0, request_limbs=classes, requests_per_pass=8, fold_columns=0,
                    workspace_bytes=0)
    wide = classes <= (4 if word_bits == 32 else 6)
    return dict(matrix_path=1, database_limbs=limbs, request_limbs=classes,
                requests_per_pass=2 * REQUEST_TILE if wide else REQUEST_TILE, fold_columns=fold_columns(limbs, environ),
                workspace_bytes=0)
