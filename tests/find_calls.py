"""The eleven C calls of the search family (include/huffman_gpu.h), described once for the tests: for each call its
arguments in order, as named slots.  tests/find_support.py fills the slots with device pointers, tests/find_args_support.py
with made-up ones.  Not a test module.

Slots: the stream head (ctx .. blocksize); what is looked for - `st` (a 32-byte set), `pattern, plen`, `cls, plen` or
`cls, lens, n` (the any-of table) -; `delims` and `words` (32-byte sets), `anchors`, `select`, `before`, `after`; the outputs
`pos`, `rlens`, `no`, `sel` with `cap` and `max_len`; the tail (counts .. hip_stream)."""
HEAD = ("ctx", "stream", "stream_len", "index", "nblocks", "sub", "raw_size", "blocksize")
TAIL = ("counts", "totals", "errs", "flags", "hip_stream")
ANY_OF = ("cls", "lens", "n")
POSITIONS = ("pos", "cap")
RECORDS = ("pos", "rlens", "cap", "max_len")

CALLS = {
    "find_bytes": HEAD + ("st",) + POSITIONS + TAIL,
    "find_pattern": HEAD + ("pattern", "plen") + POSITIONS + TAIL,
    "find_records": HEAD + ("delims", "pattern", "plen") + RECORDS + TAIL,
    "find_classes": HEAD + ("cls", "plen") + POSITIONS + TAIL,
    "find_records_classes": HEAD + ("delims", "cls", "plen") + RECORDS + TAIL,
    "find_any": HEAD + ANY_OF + POSITIONS + TAIL,
    "find_records_any": HEAD + ("delims",) + ANY_OF + RECORDS + TAIL,
    "find_records_select": HEAD + ("delims",) + ANY_OF + ("select", "pos", "rlens", "no", "cap", "max_len") + TAIL,
    "find_records_context": HEAD + ("delims",) + ANY_OF + ("select", "before", "after", "pos", "rlens", "no", "sel", "cap",
                                                            "max_len") + TAIL,
    "find_any_anchored": HEAD + ANY_OF + ("delims", "words", "anchors") + POSITIONS + TAIL,
    "find_records_anchored": HEAD + ("delims",) + ANY_OF + ("words", "anchors", "select", "before", "after", "pos", "rlens", "no",
                                                             "sel", "cap", "max_len") + TAIL,
}
RECORD_CALLS = [name for name, slots in CALLS.items() if "rlens" in slots]
ANY_OF_CALLS = [name for name, slots in CALLS.items() if "lens" in slots]


def who(name):
    """the prefix of the call's messages in hufgpu_last_error()"""
    return name + ":"


def invoke(lib, name, values):
    """the C call `name` with values[slot] in every slot of its argument list; a slot without a value is an error"""
    return getattr(lib, "hufgpu_" + name)(*[values[slot] for slot in CALLS[name]])
