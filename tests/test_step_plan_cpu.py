"""train.step_plan: which decoder-exchange scheme a step runs and the facts the step branches on, against a table written
out by hand; and the shape of PCAATrainer._step: one spine of method calls, no function defined inside another."""
import ast
import inspect

import pytest

from opensetgaitrecognition_pcaa_amd import ops, train

assert (ops.PACK_MAX_CHUNKS, ops.PACK_ROWS) == (8, 64), "the table below is written for these limits"

# (exchange, world, force_collectives, dp_zero, dp_gather, fused_decoder_update, side_streams, decoder, mode, B)
#     -> (scheme, collective, fused, exact, early, buckets)
Y, N = True, False
TABLE = [
    # single process
    ((N, 1, N, N, N, Y, Y, Y, "bf16", 64), ("none", N, Y, N, Y, N)),
    ((N, 1, N, N, N, Y, Y, Y, "fp32", 64), ("none", N, Y, Y, Y, N)),          # exact-product form of the fused update
    ((N, 1, N, N, N, Y, Y, Y, "fp16x3", 64), ("none", N, Y, Y, Y, N)),
    ((N, 1, N, N, N, N, Y, Y, "bf16", 64), ("none", N, N, N, Y, N)),          # fused update off
    ((N, 1, N, N, N, N, Y, Y, "fp32", 64), ("none", N, N, N, Y, N)),
    ((N, 1, N, N, N, N, Y, Y, "fp16x3", 64), ("none", N, N, N, Y, N)),
    ((N, 1, N, N, N, Y, N, Y, "bf16", 64), ("none", N, N, N, N, N)),          # no side streams: nothing fused, nothing early
    ((N, 1, N, N, N, Y, Y, N, "bf16", 64), ("none", N, N, N, Y, N)),          # no decoder
    ((N, 1, N, Y, N, Y, Y, Y, "bf16", 64), ("none", N, Y, N, Y, N)),          # dp_zero / dp_gather without an exchange
    ((N, 1, N, N, Y, Y, Y, Y, "bf16", 64), ("none", N, Y, N, Y, N)),
    ((Y, 1, N, N, Y, Y, Y, Y, "bf16", 64), ("none", N, Y, N, Y, N)),          # a 1-rank group, collectives not forced
    # all-reduce
    ((Y, 1, Y, N, N, Y, Y, Y, "bf16", 64), ("allreduce", Y, N, N, Y, Y)),     # forced on a 1-rank group
    ((Y, 2, N, N, N, Y, Y, Y, "bf16", 64), ("allreduce", Y, N, N, Y, Y)),
    ((Y, 2, N, N, N, Y, Y, Y, "fp32", 64), ("allreduce", Y, N, N, Y, Y)),
    ((Y, 2, N, N, N, Y, N, Y, "bf16", 64), ("allreduce", Y, N, N, N, N)),     # no wgrad stream: four chunks, Adam at the end
    # gathered operands, and each of its fallbacks
    ((Y, 8, N, N, Y, Y, Y, Y, "bf16", 64), ("gather", Y, N, N, Y, Y)),
    ((Y, 1, Y, N, Y, Y, Y, Y, "bf16", 4), ("gather", Y, N, N, Y, Y)),
    ((Y, 9, N, N, Y, Y, Y, Y, "bf16", 64), ("allreduce", Y, N, N, Y, Y)),     # world = 9
    ((Y, 8, N, N, Y, Y, Y, Y, "bf16", 65), ("allreduce", Y, N, N, Y, Y)),     # B = 65
    ((Y, 8, N, N, Y, Y, Y, Y, "fp32", 64), ("allreduce", Y, N, N, Y, Y)),     # mode fp32
    ((Y, 8, N, N, Y, N, Y, Y, "bf16", 64), ("allreduce", Y, N, N, Y, Y)),     # fused update off
    ((Y, 8, N, N, Y, Y, N, Y, "bf16", 64), ("allreduce", Y, N, N, N, N)),     # no side streams
    # sharded optimizer
    ((Y, 2, N, Y, N, Y, Y, Y, "bf16", 64), ("zero", Y, N, N, N, N)),
    ((Y, 1, Y, Y, N, Y, Y, Y, "fp32", 64), ("zero", Y, N, N, N, N)),
    ((Y, 2, N, Y, N, Y, N, Y, "bf16", 64), ("allreduce", Y, N, N, N, N)),     # zero without side streams
    ((Y, 2, N, Y, N, Y, Y, N, "bf16", 64), ("allreduce", Y, N, N, Y, Y)),     # zero without a decoder
    ((Y, 1, N, Y, N, Y, Y, Y, "bf16", 64), ("none", N, Y, N, Y, N)),          # zero on a 1-rank group, not forced
]


@pytest.mark.parametrize("args,want", TABLE)
def test_step_plan_against_the_table(args, want):
    plan = train.step_plan(*args)
    assert tuple(plan) == want
    assert plan._fields == ("scheme", "collective", "fused", "exact", "early", "buckets")


def test_every_scheme_has_a_row():
    assert {want[0] for _, want in TABLE} == {"none", "allreduce", "gather", "zero"}


def _methods():
    tree = ast.parse(inspect.getsource(train))
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PCAATrainer")
    return {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}


def _step_methods():
    """_step and the trainer methods it reaches through ``self.<method>``, transitively (finalize, which a first step runs
    once, builds the trainer and is no part of the step)"""
    methods, seen, todo = _methods(), set(), ["_step"]
    while todo:
        name = todo.pop()
        if name in seen or name == "finalize":
            continue
        seen.add(name)
        for n in ast.walk(methods[name]):
            if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "self" and n.attr in methods:
                todo.append(n.attr)
    return sorted(seen)


def test_the_step_is_split_into_methods_that_the_walk_finds():
    names = _step_methods()
    for must in ("_step", "_critic", "_critic_branch", "_decoder_backward", "_side_adam", "_bucket_hook", "_none_install",
                 "_none_update", "_allreduce_install", "_allreduce_issue", "_gather_install", "_gather_send", "_gather_update",
                 "_zero_issue", "_zero_adam", "_zero_join", "_backward_v3", "_update_encoder_and_join", "_allreduce_g"):
        assert must in names, must


def test_no_function_is_defined_inside_a_trainer_method():
    for name, node in _methods().items():
        nested = [n for n in ast.walk(node) if n is not node and isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda))]
        assert not nested, (name, [n.lineno for n in nested])


@pytest.mark.parametrize("name", _step_methods())
def test_no_code_object_among_the_constants_of_a_step_method(name):
    fn = inspect.unwrap(getattr(train.PCAATrainer, name))
    inner = [c for c in fn.__code__.co_consts if inspect.iscode(c)]
    assert not inner, (name, [c.co_name for c in inner])
