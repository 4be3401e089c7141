"""The cuckoo-table cases the CPU tests (he_keyword_pir_cuckoo_place against keyword_pir_reference.place) and the GPU tests (the
table object end to end) share.  A case is a configuration, a database of about 40 keyword-value pairs built from its seed,
and what keyword_pir_reference predicts for it: "ok", or the error's name.  test_keyword_pir.py checks every prediction against
the restatement on the CPU, so nothing here is taken from the code under test."""
import collections
import random

import keyword_pir_reference as ref

Case = collections.namedtuple("Case", "name config keywords values seed expect")


def database(seed, count=40, sizes=(0, 1, 2, 7, 8, 9, 13, 30), keyword_lengths=(0, 1, 3, 8, 21)):
    """count distinct keywords of mixed lengths with values of mixed sizes"""
    rng = random.Random(seed)
    keywords, seen = [], set()
    while len(keywords) < count:
        keyword = bytes(rng.randrange(256) for _ in range(rng.choice(keyword_lengths)))
        if keyword not in seen:
            seen.add(keyword)
            keywords.append(keyword)
    values = [bytes(rng.randrange(256) for _ in range(rng.choice(sizes))) for _ in keywords]
    return keywords, values


def _case(name, seed, expect="ok", pairs=None, **config):
    keywords, values = pairs if pairs is not None else database(seed)
    return Case(name, ref.Config(**config), keywords, values, seed, expect)


def _with_duplicates(seed):
    keywords, values = database(seed, count=34)
    # six keywords come again with other values: the first value wins
    again = keywords[3:9]
    return keywords + again, values + [b"later" + bytes([k]) for k in range(len(again))]


def _large_newcomer(seed):
    """Twenty empty values (10-byte records: nine fill a 100-byte bucket, and none can be swapped for the newcomer's 90-byte
    record), then one 80-byte value whose single candidate bucket is occupied in the first table"""
    rng = random.Random(seed)
    keywords = [bytes([k]) + bytes(rng.randrange(256) for _ in range(4)) for k in range(20)]
    return keywords + [b"the large newcomer"], [b""] * 20 + [bytes(range(80))]


LARGE_NEWCOMER = "one large newcomer, nothing to swap"

CASES = [
    _case("two tables, expansion allowed", 1, hash_function_count=2, max_eviction_count=100, max_serialized_bucket_size=100),
    _case("one table of two functions, expansion allowed", 2, hash_function_count=2, max_eviction_count=100,
          max_serialized_bucket_size=100, multiple_tables=False),
    _case("one function", 3, hash_function_count=1, max_eviction_count=10, max_serialized_bucket_size=120),
    _case("three tables, fixed size that fits", 4, hash_function_count=3, max_eviction_count=50,
          max_serialized_bucket_size=80, bucket_count=40),
    _case("one table of three functions, fixed size that fits", 5, hash_function_count=3, max_eviction_count=50,
          max_serialized_bucket_size=80, bucket_count=20, multiple_tables=False),
    _case("one slot per bucket, fixed size", 6, hash_function_count=2, max_eviction_count=100,
          max_serialized_bucket_size=100, bucket_count=128, slot_count=1),
    _case("one slot per bucket, expansion needed", 7, hash_function_count=2, max_eviction_count=20,
          max_serialized_bucket_size=200, slot_count=1),
    _case("fixed size too small", 8, expect="failedToConstructCuckooTable", hash_function_count=2, max_eviction_count=30,
          max_serialized_bucket_size=60, bucket_count=4),
    _case("duplicate keywords", 9, pairs=_with_duplicates(9), hash_function_count=2, max_eviction_count=100,
          max_serialized_bucket_size=100),
    _case("a value larger than a bucket", 10, expect="failedToConstructCuckooTable",
          pairs=(database(10)[0], database(10)[1][:39] + [bytes(200)]), hash_function_count=2, max_eviction_count=100,
          max_serialized_bucket_size=100),
    _case(LARGE_NEWCOMER, 11, pairs=_large_newcomer(11), hash_function_count=1, max_eviction_count=100,
          max_serialized_bucket_size=100, target_load_factor=0.5),
]
EXPANSION_CASES = ("one slot per bucket, expansion needed", LARGE_NEWCOMER)  # these must expand at least once
DUPLICATES_DROPPED = {"duplicate keywords": 6}
