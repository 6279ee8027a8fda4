"""CPU checks of reduced-3dgs_amd/r3dgs_model_state.py, what r3dgs_densify and r3dgs_mcmc share about the model: the entry
lists `collect` builds for the two strategies (written out here, not computed from the module), its refusals, and the
hand-over of new tensors to the model and a torch.optim.Adam that has taken one step.  Host tensors throughout: `collect`
refuses them last of all, so the tests of what it builds stand in for its device check and look at what it was asked."""
import types

import pytest
import torch

import r3dgs_model_state as ms
from tests import densify_ref

GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))
ACCUMULATORS = ("xyz_gradient_accum", "denom", "max_radii2D")
DENSIFY = ({"xyz": 2, "scaling": 3}, 1)    # r3dgs_densify: _CHILD_KIND, ZERO_NEW
MCMC = ({"opacity": 2, "scaling": 3}, 1)   # r3dgs_mcmc: _KIND, MOMENT


def _model(P=6, M=4, step=True, stateless=(), accumulators=True):
    s = densify_ref.random_state(P, M, seed=1)
    pc = types.SimpleNamespace()
    groups = []
    for name, attr in GROUPS:
        p = torch.nn.Parameter(torch.from_numpy(s[name]))
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    pc._degrees = torch.from_numpy(s["degrees"])
    if accumulators:
        for name in ACCUMULATORS:
            setattr(pc, name, torch.from_numpy(s[name]))
    pc.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if step:
        for g in groups:
            if g["name"] not in stateless:
                g["params"][0].grad = torch.full_like(g["params"][0], 0.5)
        pc.optimizer.step()
    return pc


@pytest.fixture
def device_check(monkeypatch):
    """Stands in for the refusal of host tensors; -> the list of tensor lists it was asked about."""
    asked = []
    monkeypatch.setattr(ms, "check_devices", lambda what, tensors, dev: asked.append(list(tensors)))
    return asked


def _described(pc, entries):
    """(kind, where the new tensor goes) of every entry, after checking that the entry's tensor is the one it names."""
    out = []
    for kind, t, dest in entries:
        if dest[0] == "param":
            _, group, attr, state = dest
            p = getattr(pc, attr)
            assert group["params"][0] is p and state is pc.optimizer.state.get(p) and t.data_ptr() == p.data_ptr()
            assert not t.requires_grad
            out.append((kind, "param", attr))
        elif dest[0] == "state":
            assert dest[1][dest[2]] is t
            out.append((kind, "state", [g["name"] for g in pc.optimizer.param_groups
                                        if pc.optimizer.state.get(g["params"][0]) is dest[1]][0], dest[2]))
        elif dest[0] == "grad":
            assert dest[1]["params"][0].grad is t
            out.append((kind, "grad", dest[1]["name"]))
        else:
            assert getattr(pc, dest[1]) is t
            out.append((kind,) + tuple(dest))
    return out


def test_collect_builds_the_entry_lists_of_both_strategies(device_check):
    pc = _model()
    P, dev, entries = ms.collect("densify_and_prune", pc, *DENSIFY, store_grads=False, accumulators=False)
    assert P == 6 and dev == pc._xyz.device
    assert _described(pc, entries) == [
        (2, "param", "_xyz"), (1, "state", "xyz", "exp_avg"), (1, "state", "xyz", "exp_avg_sq"),
        (0, "param", "_features_dc"), (1, "state", "f_dc", "exp_avg"), (1, "state", "f_dc", "exp_avg_sq"),
        (0, "param", "_features_rest"), (1, "state", "f_rest", "exp_avg"), (1, "state", "f_rest", "exp_avg_sq"),
        (0, "param", "_opacity"), (1, "state", "opacity", "exp_avg"), (1, "state", "opacity", "exp_avg_sq"),
        (3, "param", "_scaling"), (1, "state", "scaling", "exp_avg"), (1, "state", "scaling", "exp_avg_sq"),
        (0, "param", "_rotation"), (1, "state", "rotation", "exp_avg"), (1, "state", "rotation", "exp_avg_sq"),
        (0, "attr", "_degrees")]
    # the accumulators are checked for where they live although they are not moved
    assert len(device_check[-1]) == 19 + 3 and all(a is getattr(pc, n) for a, n in zip(device_check[-1][19:], ACCUMULATORS))
    # a bare prune with stored grads: .grad after the moments, the three accumulators last
    _, _, entries = ms.collect("prune", pc, *DENSIFY, store_grads=True, accumulators=True)
    assert _described(pc, entries) == [
        (2, "param", "_xyz"), (1, "state", "xyz", "exp_avg"), (1, "state", "xyz", "exp_avg_sq"), (1, "grad", "xyz"),
        (0, "param", "_features_dc"), (1, "state", "f_dc", "exp_avg"), (1, "state", "f_dc", "exp_avg_sq"), (1, "grad", "f_dc"),
        (0, "param", "_features_rest"), (1, "state", "f_rest", "exp_avg"), (1, "state", "f_rest", "exp_avg_sq"), (1, "grad", "f_rest"),
        (0, "param", "_opacity"), (1, "state", "opacity", "exp_avg"), (1, "state", "opacity", "exp_avg_sq"), (1, "grad", "opacity"),
        (3, "param", "_scaling"), (1, "state", "scaling", "exp_avg"), (1, "state", "scaling", "exp_avg_sq"), (1, "grad", "scaling"),
        (0, "param", "_rotation"), (1, "state", "rotation", "exp_avg"), (1, "state", "rotation", "exp_avg_sq"), (1, "grad", "rotation"),
        (0, "attr", "_degrees"), (0, "attr", "xyz_gradient_accum"), (0, "attr", "denom"), (0, "attr", "max_radii2D")]
    # MCMC: other kinds, no grads, and the accumulators are not looked at (the model need not have them)
    bare = _model(accumulators=False)
    _, _, entries = ms.collect("relocate", bare, *MCMC)
    assert _described(bare, entries) == [
        (0, "param", "_xyz"), (1, "state", "xyz", "exp_avg"), (1, "state", "xyz", "exp_avg_sq"),
        (0, "param", "_features_dc"), (1, "state", "f_dc", "exp_avg"), (1, "state", "f_dc", "exp_avg_sq"),
        (0, "param", "_features_rest"), (1, "state", "f_rest", "exp_avg"), (1, "state", "f_rest", "exp_avg_sq"),
        (2, "param", "_opacity"), (1, "state", "opacity", "exp_avg"), (1, "state", "opacity", "exp_avg_sq"),
        (3, "param", "_scaling"), (1, "state", "scaling", "exp_avg"), (1, "state", "scaling", "exp_avg_sq"),
        (0, "param", "_rotation"), (1, "state", "rotation", "exp_avg"), (1, "state", "rotation", "exp_avg_sq"),
        (0, "attr", "_degrees")]
    assert len(device_check[-1]) == 19
    # before the first step, and with one group without state: parameters only, grads only beside moments
    _, _, entries = ms.collect("prune", _model(step=False), *DENSIFY, store_grads=True, accumulators=False)
    assert [(k, d[0]) for k, _, d in entries] == [(2, "param"), (0, "param"), (0, "param"), (0, "param"), (3, "param"),
                                                  (0, "param"), (0, "attr")]
    pc = _model(stateless=("f_rest",))
    _, _, entries = ms.collect("prune", pc, *DENSIFY, store_grads=True, accumulators=False)
    assert _described(pc, entries)[4:12] == [
        (0, "param", "_features_dc"), (1, "state", "f_dc", "exp_avg"), (1, "state", "f_dc", "exp_avg_sq"), (1, "grad", "f_dc"),
        (0, "param", "_features_rest"),
        (0, "param", "_opacity"), (1, "state", "opacity", "exp_avg"), (1, "state", "opacity", "exp_avg_sq")]


def _refused(error, match, change, args=DENSIFY, **kw):
    pc = _model()
    change(pc)
    kw.setdefault("accumulators", False if args is DENSIFY else None)
    with pytest.raises(error, match=match):
        ms.collect("call", pc, *args, **kw)


def _set_state(name, key, value):
    def change(pc):
        state = pc.optimizer.state[getattr(pc, dict(GROUPS)[name])]
        if value is None:
            del state[key]
        else:
            state[key] = value
    return change


def test_collect_refuses_with_the_types_and_texts_of_the_two_strategies():
    # everything about dtype, shape and layout comes before the refusal of host tensors, which every one of these models earns
    for args in (DENSIFY, MCMC):
        _refused(RuntimeError, "call: the model has host tensors; densification needs device tensors \\(no CPU path\\)",
                 lambda pc: None, args)
        _refused(TypeError, "call: pc._xyz must be a \\[P,3\\] tensor", lambda pc: setattr(pc, "_xyz", pc._xyz.detach()[0]), args)
        _refused(ValueError, "call: the optimizer must have one single-parameter group per name in \\['f_dc', 'f_rest', 'opacity', "
                 "'rotation', 'scaling', 'xyz'\\]; found 'means' with 1 parameters",
                 lambda pc: pc.optimizer.param_groups[0].update(name="means"), args)
        _refused(ValueError, "found 'xyz' with 2 parameters",
                 lambda pc: pc.optimizer.param_groups[0]["params"].append(pc._opacity), args)
        _refused(ValueError, "call: the optimizer has no group named 'rotation'", lambda pc: pc.optimizer.param_groups.pop(), args)
        _refused(ValueError, "call: pc._opacity is not the parameter of the optimizer's group 'opacity'",
                 lambda pc: setattr(pc, "_opacity", torch.nn.Parameter(pc._opacity.detach().clone())), args)
        _refused(TypeError, "call: pc._scaling is torch.float64, expected torch.float32",
                 lambda pc: setattr(pc._scaling, "data", pc._scaling.data.double()), args)
        _refused(ValueError, "call: pc._opacity has shape \\(5, 1\\), expected \\[P, ...\\] with P = 6",
                 lambda pc: setattr(pc._opacity, "data", pc._opacity.data[:-1]), args)
        _refused(ValueError, "call: pc._rotation is not contiguous; densification takes contiguous tensors only",
                 lambda pc: setattr(pc._rotation, "data", torch.zeros(4, 6).t()), args)
        _refused(ValueError, "call: pc._rotation has shape \\(6, 3\\), expected \\(6, 4\\)",
                 lambda pc: setattr(pc._rotation, "data", torch.zeros(6, 3)), args)
        _refused(ValueError, "call: the optimizer state of group 'f_dc' has no exp_avg_sq", _set_state("f_dc", "exp_avg_sq", None), args)
        _refused(TypeError, "call: exp_avg of group 'xyz' is torch.float64, expected torch.float32",
                 _set_state("xyz", "exp_avg", torch.zeros(6, 3, dtype=torch.float64)), args)
        _refused(TypeError, "call: exp_avg of group 'xyz' must be a tensor", _set_state("xyz", "exp_avg", 0.0), args)
        _refused(ValueError, "call: exp_avg_sq of group 'opacity' has shape \\(7, 1\\), expected \\[P, ...\\] with P = 6",
                 _set_state("opacity", "exp_avg_sq", torch.zeros(7, 1)), args)
        _refused(ValueError, "call: exp_avg_sq of group 'opacity' has shape \\(6, 2\\), its parameter \\(6, 1\\)",
                 _set_state("opacity", "exp_avg_sq", torch.zeros(6, 2)), args)
        _refused(TypeError, "call: pc._degrees is torch.int64, expected torch.int32",
                 lambda pc: setattr(pc, "_degrees", pc._degrees.long()), args)
        _refused(TypeError, "call: pc._degrees must be a tensor", lambda pc: setattr(pc, "_degrees", None), args)
    _refused(ValueError, "call: store_grads=True but pc._xyz has no .grad", lambda pc: setattr(pc._xyz, "grad", None), store_grads=True)
    # (torch itself refuses a .grad of another dtype or shape than its parameter's; another layout it takes)
    _refused(ValueError, "call: pc._features_rest.grad is not contiguous",
             lambda pc: setattr(pc._features_rest, "grad", torch.zeros(6, 3, 3).transpose(1, 2)), store_grads=True)
    # densify looks at the accumulators whether it moves them or not; MCMC does not
    for moved in (False, True):
        _refused(ValueError, "call: pc.denom has shape \\(5, 1\\), expected \\[P, ...\\] with P = 6",
                 lambda pc: setattr(pc, "denom", pc.denom[:-1]), accumulators=moved)
        _refused(ValueError, "call: pc.max_radii2D has shape \\(6, 2\\), expected 6 elements",
                 lambda pc: setattr(pc, "max_radii2D", torch.zeros(6, 2)), accumulators=moved)
        _refused(TypeError, "call: pc.xyz_gradient_accum is torch.float64",
                 lambda pc: setattr(pc, "xyz_gradient_accum", pc.xyz_gradient_accum.double()), accumulators=moved)
    _refused(RuntimeError, "no CPU path", lambda pc: setattr(pc, "denom", pc.denom[:-1]), MCMC)
    # where the tensors live: host tensors first, then another device than pc._xyz's
    here, there = types.SimpleNamespace(is_cuda=True, device="cuda:0"), types.SimpleNamespace(is_cuda=True, device="cuda:1")
    ms.check_devices("call", [here, here], "cuda:0")
    with pytest.raises(ValueError, match="call: a tensor is on cuda:1, pc._xyz on cuda:0"):
        ms.check_devices("call", [here, there], "cuda:0")
    with pytest.raises(RuntimeError, match="call: noise is on cpu, pc._xyz on cuda:0; densification needs device tensors \\(no CPU path\\)"):
        ms.check_extra_device("call", "noise", torch.zeros(1), "cuda:0")
    with pytest.raises(TypeError, match="call: mask must be a torch.bool tensor"):
        ms.check_extra("call", "mask", torch.zeros(6), torch.bool, (6,), "(P,) with P = 6")
    with pytest.raises(ValueError, match="call: noise has shape \\(5, 3\\), expected \\(P, 3\\) with P = 6"):
        ms.check_extra("call", "noise", torch.zeros(5, 3), torch.float32, (6, 3), "(P, 3) with P = 6")
    with pytest.raises(ValueError, match="call: noise is not contiguous"):
        ms.check_extra("call", "noise", torch.zeros(3, 6).t(), torch.float32, (6, 3), "(P, 3) with P = 6")
    assert ms.f32(0.1) == 0.10000000149011612


@pytest.mark.parametrize("store_grads", [False, True])
def test_hand_over_rekeys_the_same_state_under_new_parameters(device_check, store_grads):
    pc = _model(stateless=("f_rest",))
    _, dev, entries = ms.collect("prune", pc, *DENSIFY, store_grads=store_grads, accumulators=True)
    old = {name: getattr(pc, attr) for name, attr in GROUPS}
    states = {name: pc.optimizer.state.get(p) for name, p in old.items()}
    steps = {name: st["step"] for name, st in states.items() if st is not None}
    assert states["f_rest"] is None and len(steps) == 5
    new = ms.new_rows(entries, 9, dev)
    assert [tuple(t.shape) for t in new] == [(9,) + tuple(e[1].shape[1:]) for e in entries]
    assert [t.dtype for t in new] == [e[1].dtype for e in entries]
    for k, t in enumerate(new):
        t.fill_(k)
    ms.hand_over(pc, entries, new)
    where = {(d[2] if d[0] == "param" else (id(d[1]),) + tuple(d[2:]) if d[0] in ("state", "grad") else d[1]): k
             for k, (_, _, d) in enumerate(entries)}   # attribute name, (id of the state dict, key), (id of the group,) -> entry
    assert len(pc.optimizer.state) == 5 and not any(p in pc.optimizer.state for p in old.values())
    for group in pc.optimizer.param_groups:
        name, attr = group["name"], dict(GROUPS)[group["name"]]
        p = group["params"][0]
        assert len(group["params"]) == 1 and p is getattr(pc, attr) and p is not old[name]
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.data_ptr() == new[where[attr]].data_ptr()
        if states[name] is None:   # a group without state moves its parameter only
            assert p not in pc.optimizer.state and p.grad is None
            continue
        st = pc.optimizer.state[p]
        assert st is states[name] and st["step"] is steps[name] and float(st["step"]) == 1.0
        assert st["exp_avg"] is new[where[id(st), "exp_avg"]] and st["exp_avg_sq"] is new[where[id(st), "exp_avg_sq"]]
        assert (p.grad is new[where[(id(group),)]]) if store_grads else p.grad is None
    for name in ("_degrees",) + ACCUMULATORS:
        assert getattr(pc, name) is new[where[name]]
    assert pc._degrees.dtype == torch.int32 and len(entries) == 6 + 10 + (5 if store_grads else 0) + 4


def test_fill_table_writes_words_kinds_and_null_for_empty_rows(device_check):
    from diff_gaussian_rasterization import _C
    pc = _model(M=1)   # sh_degree 0: _features_rest has no words
    P, dev, entries = ms.collect("add_new", pc, *MCMC)
    new = ms.new_rows(entries, 8, dev)
    table = ms.fill_table(_C._McmcTensor, entries, new, P)
    assert len(table) == len(entries) == 19
    assert [(s.row_words, s.kind) for s in table] == [(3, 0), (3, 1), (3, 1), (3, 0), (3, 1), (3, 1), (0, 0), (0, 1), (0, 1),
                                                      (1, 2), (1, 1), (1, 1), (3, 3), (3, 1), (3, 1), (4, 0), (4, 1), (4, 1), (1, 0)]
    for s, (_, t, _), out in zip(table, entries, new):
        assert (s.src, s.dst) == ((t.data_ptr(), out.data_ptr()) if s.row_words else (None, None))
