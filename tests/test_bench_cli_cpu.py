"""CPU: a plain `bench.py` run does only what its headline needs; the legs that take runs of their own (end-to-end window,
all-rows step, other operand type, CPU baseline, attention redo count) run with `--full` only."""
import ast
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP_FLAGS = ("no_e2e", "no_alt_dtype", "no_cpu_baseline")


def _parse(*argv):
    """bench.parse_args in a child process: importing bench.py sets HIP environment defaults this process must not get."""
    code = ("import json, sys, bench; a = bench.parse_args(sys.argv[1:]); "
            f"print(json.dumps({{k: getattr(a, k) for k in {('full', 'steps', 'warmup') + SKIP_FLAGS!r}}}))")
    r = subprocess.run([sys.executable, "-c", code, *argv], cwd=ROOT, capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def test_plain_run_leaves_full_off():
    a = _parse("--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a["full"] is False
    assert (a["steps"], a["warmup"]) == (7, 2)


def test_full_and_the_skip_flags_parse():
    a = _parse("--full", "--no-e2e", "--no-alt-dtype", "--no-cpu-baseline")
    assert a["full"] is True and all(a[k] for k in SKIP_FLAGS)


def test_every_extra_leg_is_gated_by_full():
    """Each `if` of main() that decides on one of the extra legs (a --no-* skip flag, or the --weights-gain redo count) also
    requires args.full."""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    legs = []
    for node in ast.walk(main):
        if isinstance(node, ast.If):
            attrs = {n.attr for n in ast.walk(node.test) if isinstance(n, ast.Attribute)}
            if attrs & set(SKIP_FLAGS) or "weights_gain" in attrs:
                legs.append((node.lineno, "full" in attrs))
    assert len(legs) >= 5, legs                     # redo count, end-to-end, all-rows, other operand type, CPU baseline
    assert all(gated for _, gated in legs), [ln for ln, gated in legs if not gated]
