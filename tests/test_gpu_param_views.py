"""Every agent form's parameter views and checkpoints, served by the library's one model table (csrc/param_table.hpp).

tools/param_view_digests.py builds the smallest agent of each of the ten forms (the candle DQN in both its forms), fills every
model through the public set_params from numpy.random.default_rng(<which id>) and saves in both checkpoint formats.
tests/golden/param_view_digests.json is that program's output at the commit BEFORE the table existed: the same values must still give
the same files, byte for byte.  On top of that, per form: load returns the bits that were set (and leaves the candle family's
target critics alone), set then get is the identity for every model and role, param_count is the sum of the model's checkpoint
tensors, refused calls change nothing, and the discrete agents still answer `which = -1` with their action count."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import param_view_digests as D  # noqa: E402

from border_amd import BdrError, _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "param_view_digests.json")))


class Case:
    def __init__(self, form, directory):
        self.form, self.dir = form, directory
        self.agent = D.build(form)
        self.views = D.views(form, self.agent)
        self.set = D.fill(self.views)                       # computed once, never changed
        self.digests = D.save_digests(self.agent, directory)

    def count_of(self, which):
        n = C.c_uint64()
        _lib.check(_lib.lib().bdr_agent_param_count_of(self.agent.handle, which, C.byref(n)))
        return n.value


@pytest.fixture(scope="module", params=D.FORMS)
def case(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp(request.param)))
    yield c
    c.agent.close()


def test_the_files_are_the_parent_commits_files_byte_for_byte(case):
    assert set(GOLDEN) == set(D.FORMS)
    assert case.digests == GOLDEN[case.form]


def test_set_then_get_is_the_identity_for_every_model_and_role(case):
    labels = [v.label for v in case.views]
    assert len(set(labels)) == len(labels) and len({v.id for v in case.views}) == len(labels)
    for v in case.views:                                   # all were set before any is read: no view aliases another
        got = v.get()
        assert got.dtype == np.float32 and got.tobytes() == case.set[v.label].tobytes(), v.label


def tensor_counts(path):
    """{tensor name: element count} of a safetensors file"""
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        head = json.loads(f.read(n))
    return {k: int(np.prod(t["shape"], dtype=np.int64)) for k, t in head.items() if k != "__metadata__"}


def file_and_prefix(form, model):
    """the checkpoint file that holds `model`'s parameters, and the prefix of its tensors in it"""
    if model.startswith("critic_"):
        return "critic", "critic%s." % model.rsplit("_", 1)[1]          # one VarMap holds every critic; the targets share their shape
    if model in D.TCH_MODELS:                                          # the optimizer arenas of the tch DQN / IQN: the online network's shape
        return "iqn" if form.startswith("iqn_") else "qnet", ""
    return {"log_alpha": "ent_coef", "policy": "policy_model"}.get(model, model), ""


def test_param_count_is_the_sum_of_the_models_checkpoint_tensors(case):
    for v in case.views:
        stem, prefix = file_and_prefix(case.form, v.model)
        sizes = tensor_counts(os.path.join(case.dir, "safetensors", stem + ".safetensors"))
        want = sum(n for k, n in sizes.items() if k.startswith(prefix))
        assert want > 0 and case.count_of(v.id) == want == case.set[v.label].size, v.label


@pytest.mark.parametrize("fmt", D.FORMATS)
def test_load_returns_the_bits_that_were_set(case, fmt):
    saved = [v for v in case.views if v.saved]
    other = [v for v in case.views if not v.saved]
    for v in saved:
        v.set(np.full(case.set[v.label].size, 7.0, np.float32))
    case.agent.set_checkpoint_format(fmt)
    case.agent.load_params(os.path.join(case.dir, fmt))
    for v in saved:
        assert v.get().tobytes() == case.set[v.label].tobytes(), v.label
    for v in other:                                        # among them the candle family's target critics: critic.tgt goes into the ONLINE critics
        assert v.get().tobytes() == case.set[v.label].tobytes(), v.label
    if case.form in D.CANDLE_CRITICS:
        assert any(v.model.startswith("critic_tgt_") for v in other)


def test_refused_calls_raise_and_change_nothing(case):
    h, v = case.agent.handle, case.views[0]
    before = v.get()
    buf = np.zeros(before.size + 1, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    lib = _lib.lib()
    for call in (lambda: lib.bdr_agent_set_params(h, 77, ptr, before.size), lambda: lib.bdr_agent_get_params(h, 77, ptr, before.size),
                 lambda: lib.bdr_agent_set_params(h, v.id, ptr, before.size + 1), lambda: lib.bdr_agent_get_params(h, v.id, ptr, before.size - 1)):
        with pytest.raises(BdrError):
            _lib.check(call())
    assert case.count_of(77) == 0
    assert (buf == 0).all() and v.get().tobytes() == before.tobytes()


def test_discrete_agents_answer_minus_one_with_their_action_count(case):
    assert case.count_of(-1) == D.DISCRETE.get(case.form, 0)


@pytest.mark.parametrize("form", ("candle_dqn_mlp", "candle_dqn_cnn"))
def test_the_candle_dqn_serves_one_arena_under_the_tch_number_and_the_role(form):
    """CandleDqn::slot takes exp_avg as 2 and 200, exp_avg_sq as 3 and 300, grad as 4 and 100 (the Python class asks with the tch
    numbers only): set through one id, read through the other, in both directions"""
    agent = D.build(form)
    lib, h, n = _lib.lib(), agent.handle, agent.param_count()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for tch, role in ((2, 200), (3, 300), (4, 100)):
        for setter, getter in ((role, tch), (tch, role)):
            vals, out = np.random.default_rng(setter).standard_normal(n, dtype=np.float32), np.zeros(n, np.float32)
            _lib.check(lib.bdr_agent_set_params(h, setter, ptr(vals), n))
            _lib.check(lib.bdr_agent_get_params(h, getter, ptr(out), n))
            assert out.tobytes() == vals.tobytes(), (setter, getter)
            count = C.c_uint64()
            _lib.check(lib.bdr_agent_param_count_of(h, getter, C.byref(count)))
            assert count.value == n
    agent.close()


def test_the_tch_dqn_forgets_its_weight_planes_when_qnet_is_set():
    """set_params("qnet") after a forward, then qvalues == qvalues of a fresh agent given the same parameters: the bf16 planes split
    from the old parameters were marked stale (DqnCnn::params_written).  9 rows: up to 8 the acting kernels answer, which read the
    f32 weights; from 9 on qvalues is the training forward, whose conv2 / conv3 read the planes.  (With planes_stale taken out of
    params_written this test fails: the used agent answers with conv2 / conv3 of its old parameters.)"""
    rng = np.random.default_rng(5)
    obs = rng.integers(0, 256, (9, 1, 84, 84), dtype=np.uint8)
    used, fresh = D.build("dqn_cnn"), D.build("dqn_cnn")
    p = (0.05 * rng.standard_normal(used.param_count())).astype(np.float32)
    q_old = used.qvalues(obs)                               # splits the planes of the initial parameters
    used.set_params(p, "qnet")
    fresh.set_params(p, "qnet")
    q = used.qvalues(obs)
    assert q.tobytes() == fresh.qvalues(obs).tobytes() and q.tobytes() != q_old.tobytes()
    used.close(), fresh.close()
