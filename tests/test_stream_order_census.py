"""No GPU: the table of the stream-order tests (tests/helpers/stream_order_cases.py) covers every public call of
nvimagecodec_amd.lowlevel that takes a `stream`, and every test it names exists in tests/test_gpu_stream_order.py."""
import ast
import inspect
import os

from helpers.stream_order_cases import CASES, EXEMPT, PLUGIN_CASES
from nvimagecodec_amd import lowlevel


def _stream_takers():
    found = set()
    for cname, cls in inspect.getmembers(lowlevel, inspect.isclass):
        if cls.__module__ != lowlevel.__name__:
            continue
        for mname, fn in inspect.getmembers(cls, inspect.isfunction):
            if not mname.startswith("_") and "stream" in inspect.signature(fn).parameters:
                found.add(cname + "." + mname)
    return found


def test_every_stream_parameter_is_covered_or_exempt_with_a_reason():
    takers = _stream_takers()
    assert len(takers) >= 16 and "BatchDecoder.decode" in takers  # (the walk itself works)
    assert not set(CASES) & set(EXEMPT)
    missing = takers - set(CASES) - set(EXEMPT)
    assert not missing, "calls with a `stream` parameter that tests/helpers/stream_order_cases.py does not know: %s" % sorted(missing)
    stale = (set(CASES) | set(EXEMPT)) - takers
    assert not stale, "entries for calls that no longer take a stream: %s" % sorted(stale)
    for name, (checks, tests) in list(CASES.items()) + list(PLUGIN_CASES.items()):
        assert set(checks) <= set("PWC") and tests, name
    for name, reason in EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, name


def test_every_test_the_table_names_exists():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_stream_order.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    named = {t for _, tests in list(CASES.values()) + list(PLUGIN_CASES.values()) for t in tests}
    assert named <= defined, sorted(named - defined)
    # and the other way round: no stream-order test without a line in the table
    assert {d for d in defined if d.startswith("test_")} <= named, sorted({d for d in defined if d.startswith("test_")} - named)
    # the rule of tests/helpers/stalled_stream.py: one device-wide synchronise (ready()), none in the tests themselves
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "synchronize"]
    for c in calls:
        owner = c.func.value
        assert not (isinstance(owner, ast.Attribute) and owner.attr == "cuda"), "torch.cuda.synchronize() in line %d" % c.lineno
