"""Request bodies for the native /score JSON parser (csrc/host_codec.h), all
generated in code and deterministic: truncations and single-byte mutations of
valid bodies, number literals, strings and escapes, structure, and seeded
random valid bodies. ``corpus()`` returns ``[(name, body bytes), ...]``; the
name's first component is the group. tests/test_host_codec.py runs every body
through the stand-alone harness and through the pydantic path.

The vocabularies are fixed here (not taken from a trained model) so that the
corpus and the expected arrays do not depend on a training run.
"""

from __future__ import annotations

import functools
import json
import random

from creditcore.data import VOCABULARIES
from creditcore.schema import (
    CATEGORICAL_FEATURES,
    FEATURES,
    MISSING_CATEGORY,
    NUMERIC_FEATURES,
    SAMPLE_REQUEST,
)

VOCABS: list[list[str]] = [
    sorted(VOCABULARIES[c] + [MISSING_CATEGORY]) for c in CATEGORICAL_FEATURES
]

# The bytes put at every position of the one-record body.
MUTATION_BYTES = [ord(c) for c in '"\\{}[],:'] + [0x00, 0x1F, 0x7F, 0x80, 0xFF]

# Ignored values: nested containers with brackets and quotes inside strings.
_EXTRA_1 = {"note": ["]", "}", '"', "\\", "[{"]}
_EXTRA_2 = {"tags": [{"k": "a]b", "v": [1, 2.5, None, True, {}]}, []], "s": '}"{'}


def _dumps(obj, **kw) -> bytes:
    return json.dumps(obj, **kw).encode()


def _record(rng: random.Random) -> dict:
    rec = {}
    for c, vocab in zip(CATEGORICAL_FEATURES, VOCABS):
        rec[c] = rng.choice(vocab)
    for c in NUMERIC_FEATURES:
        rec[c] = round(rng.uniform(0.0, 50000.0), 2)
    rec["age"] = float(rng.randrange(21, 75))
    return rec


def base_one() -> bytes:
    """One full record in schema order (the sample request)."""
    return _dumps(SAMPLE_REQUEST)


def base_shuffled() -> bytes:
    """One record, fields shuffled, with extra (ignored) fields among them."""
    rng = random.Random(11)
    items = list(_record(rng).items()) + [("extra_a", _EXTRA_1), ("extra_b", _EXTRA_2),
                                          ("extra_c", None), ("", -1.5e-3)]
    rng.shuffle(items)
    return _dumps([dict(items)])


def base_three() -> bytes:
    rng = random.Random(12)
    return _dumps([_record(rng) for _ in range(3)])


BASE = {"base/one": base_one, "base/shuffled": base_shuffled, "base/three": base_three}


def _truncations():
    for name, make in BASE.items():
        body = make()
        for n in range(len(body)):  # every proper prefix; the whole is base/*
            yield f"trunc/{name[5:]}/{n}", body[:n]


def _mutations():
    body = base_one()
    for i in range(len(body)):
        for b in MUTATION_BYTES:
            if body[i] != b:
                yield f"mut/{i}/{b:02x}", body[:i] + bytes([b]) + body[i + 1:]


NUMBER_LITERALS = [
    "nan", "inf", "-inf", "nan(1)", "01", "1.", ".5", "-.5",
    "-", "-0", "0e0", "1e309", "1e-400", "1E+2", "1" * 400, "+1", "0x10", "1 2",
    # the spellings the pydantic path takes besides JSON's own
    "NaN", "Infinity", "-Infinity", "-NaN", "+Infinity", "infinity", "Inf",
    # JSON numbers and near misses
    "0", "-0.0", "0.5", "-1", "10", "1e5", "1E5", "1e+5", "1e-5", "1.5e3", "0.0e-0",
    "1e", "1e+", "1.e5", "1.5e", "-01", "00", "0.", "1..5", "1.5.5", "1e5.5", "--1",
    "1-", "1e5e5", "0e", "1_000", "1,5", "1f", "1d", "0b1", "1e0x1", "١",
    "4.9e-324", "2.2250738585072014e-308", "1e-45", "1.401298464324817e-45",
    "3.4028234663852886e38", "3.4028235677973366e38", "3.5e38", "1.7976931348623157e308",
    "-1e309", "16777217", "9007199254740993", "123456789012345678901234567890",
    "0.1" + "0" * 300, "0." + "0" * 400 + "1",
]


def _numbers():
    lits = [lit.encode() for lit in NUMBER_LITERALS]
    for k, enc in enumerate(lits):
        yield f"num/field/{k}", b'[{"age": ' + enc + b"}]"
    for k, enc in enumerate(lits):
        yield f"num/ignored/{k}", b'[{"zz": ' + enc + b', "age": 3}]'
        yield f"num/nested/{k}", b'[{"zz": [' + enc + b"]}]"
        yield f"num/last/{k}", b'[{"age": ' + enc  # the literal ends the buffer


def _in_string_positions(tag: str, inner: bytes):
    """inner (raw bytes between the quotes) as a categorical value, as an
    ignored value, nested in an ignored value, and as a key."""
    yield f"str/{tag}/cat", b'[{"sex": "' + inner + b'"}]'
    yield f"str/{tag}/ignored", b'[{"zz": "' + inner + b'", "age": 3}]'
    yield f"str/{tag}/nested", b'[{"zz": {"a": ["' + inner + b'"]}}]'
    yield f"str/{tag}/key", b'[{"' + inner + b'": 1, "age": 3}]'
    yield f"str/{tag}/nestedkey", b'[{"zz": {"' + inner + b'": 1}}]'


def _hash_twins() -> list[tuple[str, str]]:
    """Schema keys that share length and last character, which is all the
    parser's dispatch hash looks at."""
    out = []
    for i, a in enumerate(FEATURES):
        for b in FEATURES[i + 1:]:
            if len(a) == len(b) and a[-1] == b[-1]:
                out.append((a, b))
    return out


def _strings():
    for c in '"\\/bfnrtu' + "aUx0'vN ":
        yield from _in_string_positions(f"esc_{ord(c):02x}", b"a\\" + c.encode() + b"b")
    for n in range(5):
        hexd = b"0041"[:n]
        yield from _in_string_positions(f"u{n}", b"\\u" + hexd)
        yield from _in_string_positions(f"u{n}_mid", b"x\\u" + hexd + b"x")
    for tag, inner in [
        ("u_upper", b"\\u00E9"), ("u_lower", b"\\u00e9"), ("u_bad_hex", b"\\u00g0"),
        ("u_bad_hex4", b"\\u000g"), ("u_sign", b"\\u+041"), ("u_zero", b"\\u0000"),
        ("u_3byte", b"\\u20ac"), ("u_ffff", b"\\uffff"),
        ("pair", b"\\ud83d\\ude00"), ("pair_upper", b"\\uD83D\\uDE00"),
        ("lone_high", b"\\ud83d"), ("lone_low", b"\\ude00"),
        ("high_then_bmp", b"\\ud83d\\u0041"), ("high_then_char", b"\\ud83dx"),
        ("high_then_high", b"\\ud83d\\ud83d"), ("low_then_high", b"\\ude00\\ud83d"),
        ("high_then_backslash", b"\\ud83d\\n"), ("high_then_short", b"\\ud83d\\ude0"),
        ("ctl_01", b"a\x01b"), ("ctl_00", b"\x00"), ("ctl_1f", b"\x1f"),
        ("ctl_tab", b"a\tb"), ("ctl_nl", b"a\nb"), ("ctl_cr", b"\r"),
        ("del_7f", b"a\x7fb"),
        ("utf8_2", "é".encode()), ("utf8_3", "€".encode()), ("utf8_4", "😀".encode()),
        ("utf8_bom", b"\xef\xbb\xbf"), ("utf8_max", b"\xf4\x8f\xbf\xbf"),
        ("bad_ff", b"\xff"), ("bad_fe", b"a\xfeb"), ("bad_lead_alone", b"\xc3"),
        ("bad_cont_alone", b"\x80"), ("bad_c3_28", b"\xc3\x28"),
        ("bad_trunc3", b"\xe2\x82"), ("bad_trunc4", b"\xf0\x9f\x98"),
        ("bad_e2_28", b"\xe2\x28\xa1"), ("overlong2", b"\xc0\xaf"), ("overlong_c1", b"\xc1\xbf"),
        ("overlong3", b"\xe0\x80\xaf"), ("overlong4", b"\xf0\x80\x80\xaf"),
        ("surrogate_raw", b"\xed\xa0\x80"), ("above_10ffff", b"\xf4\x90\x80\x80"),
        ("lead_f5", b"\xf5\x80\x80\x80"), ("lead_f8", b"\xf8\x88\x80\x80\x80"),
        ("quote_esc_end", b"abc\\\""), ("backslash_pair", b"\\\\"),
        ("backslash_pair_quote", b"\\\\\\\""),
    ]:
        yield from _in_string_positions(tag, inner)
    # a backslash as the body's last byte
    for k, body in enumerate([b'[{"sex": "abc\\', b'[{"sex": "\\', b'[{"a\\', b'[{"zz": "\\',
                              b'[{"zz": ["\\', b'[{"sex": "male"}]\\', b'[{"sex": "a\\u00',
                              b'[{"sex": "a\\u', b'[{"sex": "a\\\\']):
        yield f"str/last_backslash/{k}", body
    # vocabulary words and keys spelled with escapes
    for k, (key, val) in enumerate([
        ("sex", "m\\u0061le"), ("sex", "\\u006d\\u0061\\u006c\\u0065"), ("sex", "\\u006Dale"),
        ("sex", "fem\\u0061le"), ("sex", "ma\\/le"), ("sex", "male\\u0000"),
        ("repayment_status_1", "duly\\u005fpaid"), ("education", "high\\u005Fschool"),
        ("s\\u0065x", "female"), ("credit\\u005flimit", None), ("a\\u0067e", None),
        ("\\u0061\\u0067\\u0065", None), ("ag\\/e", None), ("age\\u0000", None),
        ("payment_amount_\\u0036", None), ("s\\u0065x", "f\\u0065male"),
    ]):
        v = b'"' + val.encode() + b'"' if val is not None else b"41.5"
        yield f"str/escaped_word/{k}", b'[{"' + key.encode() + b'": ' + v + b"}]"
    # 63, 64 and 65 bytes after unescaping, the size of the parser's buffers,
    # with the last character of one, two, three and four bytes
    for n in (63, 64, 65):
        for tag, tail, tail_len in [("plain", b"", 0), ("esc1", b"\\u0041", 1), ("esc_n", b"\\n", 1),
                                    ("esc2", b"\\u00e9", 2), ("esc3", b"\\u20ac", 3),
                                    ("pair", b"\\ud83d\\ude00", 4)]:
            inner = b"a" * (n - tail_len) + tail
            yield from _in_string_positions(f"len{n}_{tag}", inner)
            yield from _in_string_positions(f"len{n}_{tag}_front", tail + b"a" * (n - tail_len))
    yield "str/empty_key/num", b'[{"": 1, "age": 3}]'
    yield "str/empty_key/str", b'[{"": "x"}]'
    yield "str/empty_key/only", b'[{"": {}}]'
    yield "str/empty_key/escaped_empty", b'[{"\\u0000": 1}]'
    yield "str/empty_value/cat", b'[{"sex": ""}]'
    # the dispatch hash: schema keys that collide (none do in this schema, so
    # this loop is empty today) and near misses that collide with a schema key
    for k, (a, b) in enumerate(_hash_twins()):
        yield f"str/hash_twin/{k}", _dumps([{a: 1.5, b: 2.5}])
        yield f"str/hash_twin_rev/{k}", _dumps([{b: 2.5, a: 1.5}])
    for k, key in enumerate(["sox", "abe", "bge", "kill_amount_1", "bill_amounx_1", "xill_amount_6",
                             "credit_limiT", "credit-limit", "Sex", "sex ", " sex", "se",
                             "sexx", "payment_amount_7", "payment_amount_", "repayment_status_0"]):
        yield f"str/hash_near/{k}", _dumps([{key: 7, "age": 3}])
        yield f"str/hash_near_first/{k}", _dumps([{"sex": "female", key: "female", "age": 3}])


def _nest(depth: int, open_: bytes, close: bytes, core: bytes = b"") -> bytes:
    return b'[{"zz": ' + open_ * depth + core + close * depth + b', "age": 3}]'


def _structure():
    rng = random.Random(13)
    full = _record(rng)
    cases = {
        "dup/num": b'[{"age": 1, "age": 2}]',
        "dup/cat": b'[{"sex": "male", "sex": "female"}]',
        "dup/first_bad": b'[{"age": "x", "age": 1}]',
        "dup/last_bad": b'[{"age": 1, "age": null}]',
        "dup/ignored": b'[{"zz": 1, "zz": [2], "age": 3}]',
        "dup/apart": b'[{"age": 1, "sex": "female", "age": 2, "sex": "male"}]',
        "reverse": _dumps([dict(reversed(list(full.items())))]),
        "absent/one": b"[{}]",
        "absent/two": b"[{}, {}]",
        "absent/extra_only": b'[{"zz": 1}]',
        "absent/ws": b"[ { } ]",
        "mismatch/issue": b'[{"x": [}]}]',
        "mismatch/obj_arr": b'[{"x": {]}]',
        "mismatch/deep": b'[{"x": [1, {"a": 2]}]}]',
        "mismatch/then_field": b'[{"x": [}], "age": 1}]',
        "mismatch/top_a": b'[{"age": 1]}',
        "mismatch/top_b": b'[{"age": 1}}',
        "mismatch/top_c": b'{"age": 1}]',
        "mismatch/crossed": b'[{"x": [{]}}]',
        "mismatch/extra_close": b'[{"x": []]}]',
        "mismatch/extra_open": b'[{"x": [[]}]',
        "comma/obj": b'[{"age": 1,}]',
        "comma/arr": b'[{"age": 1},]',
        "comma/ignored_arr": b'[{"x": [1,]}]',
        "comma/ignored_obj": b'[{"x": {"a": 1,}}]',
        "comma/only": b"[,]",
        "comma/obj_only": b"[{,}]",
        "comma/leading": b'[{,"age": 1}]',
        "comma/double": b'[{"age": 1,, "sex": "male"}]',
        "comma/missing": b'[{"age": 1 "sex": "male"}]',
        "comma/missing_rows": b"[{} {}]",
        "comma/ignored_leading": b'[{"x": [,1]}]',
        "comma/ignored_missing": b'[{"x": [1 2]}]',
        "comma/ignored_obj_missing": b'[{"x": {"a": 1 "b": 2}}]',
        "ignored/bare_word": b'[{"x": {a}}]',
        "ignored/key_only": b'[{"x": {"a"}}]',
        "ignored/no_value": b'[{"x": {"a":}}]',
        "ignored/num_key": b'[{"x": {1: 2}}]',
        "ignored/colon_in_arr": b'[{"x": [1: 2]}]',
        "ignored/lone_colon": b'[{"x": [:]}]',
        "ignored/nul": b'[{"x": [nul]}]',
        "ignored/tru": b'[{"x": tru}]',
        "ignored/nulll": b'[{"x": nulll}]',
        "ignored/True": b'[{"x": True}]',
        "ignored/leading_zero": b'[{"x": [01]}]',
        "ignored/two_values": b'[{"x": 1 2}]',
        "ignored/str_no_comma": b'[{"x": ["a" "b"]}]',
        "ignored/obj_in_arr_colon": b'[{"x": ["a": 1]}]',
        "ignored/value_in_obj": b'[{"x": {"a", "b"}}]',
        "ignored/empty": b'[{"x": }]',
        "ignored/ok_mixed": b'[{"x": [null, true, false, 1, -2.5e-3, "s", {}, [], {"a": []}], "age": 3}]',
        "bom/front": b"\xef\xbb\xbf" + base_one(),
        "bom/front_empty": b"\xef\xbb\xbf[]",
        "bom/back": b"[{}]\xef\xbb\xbf",
        "bom/inside": b"[\xef\xbb\xbf{}]",
        "bom/utf16": "[{}]".encode("utf-16"),
        "empty/body": b"",
        "empty/array": b"[]",
        "empty/array_ws": b" [ ] ",
        "empty/ws_only": b" \n",
        "top/null": b"null",
        "top/object": b"{}",
        "top/record": b'{"age": 1}',
        "top/number_row": b"[1]",
        "top/array_row": b"[[]]",
        "top/null_row": b"[null]",
        "top/string_row": b'["x"]',
        "top/string": b'"x"',
        "top/trailing_word": b"[{}] x",
        "top/two_docs": b"[{}][{}]",
        "top/trailing_comma_doc": b"[{}],",
        "top/trailing_nul": b"[{}]\x00",
        "top/nested_rows": b"[[{}]]",
        "colon/missing": b'[{"sex" "male"}]',
        "colon/double": b'[{"age":: 1}]',
        "colon/equals": b'[{"age" = 1}]',
        "colon/no_value": b'[{"age": }]',
        "colon/no_value_end": b'[{"age":',
        "key/unquoted": b"[{age: 1}]",
        "key/single_quoted": b"[{'age': 1}]",
        "key/number": b"[{1: 1}]",
        "key/null": b"[{null: 1}]",
        "value/single_quoted": b"[{\"sex\": 'male'}]",
    }
    for name, body in cases.items():
        yield f"struct/{name}", body
    # null, true, false, a string, a number, an object and an array for each
    # kind of field
    for kind, key in (("cat", "sex"), ("num", "age"), ("ignored", "zz")):
        for tag, lit in (("null", "null"), ("true", "true"), ("false", "false"),
                         ("string", '"male"'), ("numeric_string", '"33"'), ("number", "33"),
                         ("float", "33.5"), ("object", "{}"), ("array", "[]"),
                         ("array_of_one", "[33]"), ("nul", "nul"), ("n", "n"),
                         ("nullx", "nullx"), ("Null", "Null")):
            yield f"struct/kind/{kind}/{tag}", ('[{"%s": %s}]' % (key, lit)).encode()
            yield f"struct/kind/{kind}/{tag}/then", ('[{"%s": %s, "marriage": "single"}]' % (key, lit)).encode()
    for depth in (1, 2, 3, 50, 99, 100, 101, 127, 128, 129, 199, 200, 201, 255, 256, 257, 1000):
        yield f"struct/nest/arr/{depth}", _nest(depth, b"[", b"]")
        yield f"struct/nest/obj/{depth}", _nest(depth, b'{"a": ', b"}", b"1")
        yield f"struct/nest/mixed/{depth}", _nest(depth, b'[{"]}\\"[": ', b"}]", b'"[{\\"]"')
    yield "struct/nest/unclosed/1000", b'[{"zz": ' + b"[" * 1000
    yield "struct/nest/overclosed", b'[{"zz": [[]]]}]'
    # whitespace: JSON's four bytes between all tokens, then bytes that are
    # whitespace elsewhere but not in JSON
    toks = [b"[", b"{", b'"sex"', b":", b'"female"', b",", b'"zz"', b":", b"[", b"1", b",",
            b"{", b'"a"', b":", b"null", b"}", b"]", b",", b'"age"', b":", b"-2.5e1", b"}",
            b",", b"{", b"}", b"]"]
    for tag, w in (("space", b" "), ("tab", b"\t"), ("nl", b"\n"), ("cr", b"\r"), ("all", b" \t\n\r"),
                   ("vt", b"\v"), ("ff", b"\f"), ("nbsp", b"\xc2\xa0"), ("nul", b"\x00"),
                   ("a0", b"\xa0"), ("bs", b"\b"), ("none", b"")):
        yield f"struct/ws/{tag}", w + w.join(toks) + w
    for tag, w in (("vt", b"\v"), ("ff", b"\f")):
        for k in range(len(toks) + 1):
            yield f"struct/ws/{tag}_at/{k}", b"".join(toks[:k]) + w + b"".join(toks[k:])
    yield "struct/ws/in_number", b'[{"age": 1 .5}]'
    yield "struct/ws/in_literal", b'[{"zz": nu ll}]'
    yield "struct/ws/minus_space", b'[{"age": - 1}]'


def _number_text(rng: random.Random) -> str:
    kind = rng.randrange(8)
    if kind == 0:
        return str(rng.randrange(-10**6, 10**6))
    if kind == 1:
        return repr(round(rng.uniform(-1e5, 1e5), rng.randrange(0, 6)))
    if kind == 2:
        return repr(rng.uniform(-1.0, 1.0) * 10.0 ** rng.randrange(-30, 30))
    if kind == 3:  # exponents spelled the ways JSON allows
        m = rng.choice(["1", "2.5", "-7", "0.125", "-0.5", "12345.678"])
        e = rng.choice(["e", "E"]) + rng.choice(["", "+", "-"]) + str(rng.randrange(0, 20))
        return m + e
    if kind == 4:  # denormals, of float64 and of float32
        return rng.choice(["4.9e-324", "5e-324", "1e-310", "2.2e-308", "-3e-320",
                           "1e-40", "1.4e-45", "-7e-46", "1e-60"])
    if kind == 5:  # at and past the float32 range
        return rng.choice(["", "-"]) + repr(rng.uniform(1.0, 10.0)) + "e38"
    if kind == 6:
        return rng.choice(["0", "-0", "0.0", "-0.0", "0e0", "0.0E-5", "1e0"])
    return str(rng.randrange(0, 10**18))


def _random_valid():
    for seed in range(200):
        rng = random.Random(1000 + seed)
        rows = []
        for _ in range(rng.randrange(1, 6)):
            items = []
            for c, vocab in zip(CATEGORICAL_FEATURES, VOCABS):
                if rng.random() < 0.2:
                    continue
                word = rng.choice(vocab) if rng.random() < 0.85 else rng.choice(
                    ["", "phd", "Male", "duly paid", "né", "x" * 70])
                items.append(json.dumps(c) + ": " + json.dumps(word, ensure_ascii=rng.random() < 0.5))
            for c in NUMERIC_FEATURES:
                if rng.random() < 0.2:
                    continue
                items.append(json.dumps(c) + ": " + _number_text(rng))
            for k in range(rng.randrange(0, 3)):
                extra = rng.choice([_EXTRA_1, _EXTRA_2, None, True, 12, "s]", [[], {}], -0.5])
                items.append(json.dumps(f"extra_{k}") + ": " + json.dumps(extra))
            if rng.random() < 0.7:
                rng.shuffle(items)
            sep = rng.choice([", ", ",", " ,\n  "])
            rows.append("{" + sep.join(items) + "}")
        body = "[" + rng.choice([", ", ",", ",\n"]).join(rows) + "]"
        yield f"rand/{seed}", body.encode()


# Cases the fast path exists for: it must take them.
def must_accept(name: str) -> bool:
    return name.startswith(("base/", "rand/"))


@functools.lru_cache(maxsize=None)
def corpus() -> tuple[tuple[str, bytes], ...]:
    out = [(name, make()) for name, make in BASE.items()]
    for gen in (_truncations, _mutations, _numbers, _strings, _structure, _random_valid):
        out.extend(gen())
    names = [n for n, _ in out]
    assert len(set(names)) == len(names), "duplicate case name"
    return tuple(out)
