"""`r3dgs_model_state` -- what the densification strategies (r3dgs_densify, r3dgs_mcmc) share about a model shaped like the
reference's GaussianModel: the checks of its tensors, the list of tensors a move launch takes, and the hand-over of the new
tensors to the model and its optimizer.

`pc` has `_xyz`, `_features_dc`, `_features_rest`, `_opacity`, `_scaling`, `_rotation`, `_degrees` and `optimizer`, whose groups
are named as in GROUPS with one parameter each.  An entry is (kind, source tensor, where its new tensor goes): kind is the
strategy's word for how new rows are made (R3DGS_DENSIFY_* / R3DGS_MCMC_*, 0 = a plain copy in both), the destination one of
("param", group, attr, state), ("state", state dict, key), ("grad", group), ("attr", name)."""
import numpy as np
import torch
from torch import nn

GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))
NAMES = {name for name, _ in GROUPS}
WIDTHS = {"xyz": (3,), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
ACCUMULATORS = ("xyz_gradient_accum", "denom", "max_radii2D")
COPY, MAX_TENSORS = 0, 32     # R3DGS_{DENSIFY,MCMC}_COPY, _MAX_TENSORS


def check(what, name, t, dtype, P):
    """dtype and shape first, so that a wrong tensor is named for what is wrong with it wherever it lives"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {name} is {t.dtype}, expected {dtype}")
    if t.dim() < 1 or t.shape[0] != P:
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected [P, ...] with P = {P}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} is not contiguous; densification takes contiguous tensors only")


def check_extra(what, name, t, dtype, shape, shape_text):
    """noise, uniforms and mask: looked at before the model's tensors, except for where they live"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{what}: {name} must be a {dtype} tensor")
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {shape_text}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} is not contiguous; densification takes contiguous tensors only")


def check_extra_device(what, name, t, dev):
    if t.device != dev:
        raise RuntimeError(f"{what}: {name} is on {t.device}, pc._xyz on {dev}; densification needs device tensors "
                           "(no CPU path)")


def check_devices(what, tensors, dev):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{what}: the model has host tensors; densification needs device tensors (no CPU path)")
        if t.device != dev:
            raise ValueError(f"{what}: a tensor is on {t.device}, pc._xyz on {dev}")


def model_size(what, pc):
    xyz = pc._xyz
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2:
        raise TypeError(f"{what}: pc._xyz must be a [P,3] tensor")
    return xyz.shape[0]


def f32(x):
    """a Python double rounded to float32 once, as torch rounds the scalar it compares a float32 tensor with"""
    return float(np.float32(x))


def collect(what, pc, param_kinds, moment_kind, store_grads=False, accumulators=None):
    """-> (P, device, entries), in table order: every parameter followed by its two moments (kind moment_kind) and, with
    store_grads, its .grad, if its group has state; then _degrees.  param_kinds: {group name: kind}, a plain copy otherwise.
    accumulators: None leaves ACCUMULATORS alone; False checks them; True also adds them to the entries.  Every refusal
    comes from here, before anything is launched or changed: dtypes, shapes and layouts of all tensors first, then where
    they live."""
    P = model_size(what, pc)
    groups = {}
    for group in pc.optimizer.param_groups:
        name = group.get("name")
        if name not in NAMES or len(group["params"]) != 1:
            raise ValueError(f"{what}: the optimizer must have one single-parameter group per name in {sorted(NAMES)}; "
                             f"found {name!r} with {len(group['params'])} parameters")
        groups[name] = group
    entries = []
    for name, attr in GROUPS:
        if name not in groups:
            raise ValueError(f"{what}: the optimizer has no group named {name!r}")
        group = groups[name]
        p = group["params"][0]
        if getattr(pc, attr) is not p:
            raise ValueError(f"{what}: pc.{attr} is not the parameter of the optimizer's group {name!r}")
        check(what, f"pc.{attr}", p, torch.float32, P)
        if name in WIDTHS and tuple(p.shape[1:]) != WIDTHS[name]:
            raise ValueError(f"{what}: pc.{attr} has shape {tuple(p.shape)}, expected {(P,) + WIDTHS[name]}")
        state = pc.optimizer.state.get(p, None)
        entries.append((param_kinds.get(name, COPY), p.detach(), ("param", group, attr, state)))
        if state is None:
            continue
        for key in ("exp_avg", "exp_avg_sq"):
            if key not in state:
                raise ValueError(f"{what}: the optimizer state of group {name!r} has no {key}")
            check(what, f"{key} of group {name!r}", state[key], torch.float32, P)
            if state[key].shape != p.shape:
                raise ValueError(f"{what}: {key} of group {name!r} has shape {tuple(state[key].shape)}, its parameter "
                                 f"{tuple(p.shape)}")
            entries.append((moment_kind, state[key], ("state", state, key)))
        if store_grads:
            if p.grad is None:
                raise ValueError(f"{what}: store_grads=True but pc.{attr} has no .grad")
            check(what, f"pc.{attr}.grad", p.grad, torch.float32, P)
            if p.grad.shape != p.shape:
                raise ValueError(f"{what}: pc.{attr}.grad has shape {tuple(p.grad.shape)}, its parameter {tuple(p.shape)}")
            entries.append((moment_kind, p.grad, ("grad", group)))
    check(what, "pc._degrees", pc._degrees, torch.int32, P)
    entries.append((COPY, pc._degrees, ("attr", "_degrees")))
    checked = []
    for name in ACCUMULATORS if accumulators is not None else ():
        t = getattr(pc, name)
        check(what, f"pc.{name}", t, torch.float32, P)
        if t.numel() != P:
            raise ValueError(f"{what}: pc.{name} has shape {tuple(t.shape)}, expected {P} elements")
        checked.append(t)
        if accumulators:
            entries.append((COPY, t, ("attr", name)))
    dev = pc._xyz.device
    check_devices(what, [e[1] for e in entries] + checked, dev)
    if len(entries) > MAX_TENSORS:
        raise RuntimeError(f"{what}: more than {MAX_TENSORS} tensors")
    return P, dev, entries


def new_rows(entries, rows, dev):
    """-> an empty tensor of `rows` rows for every entry, of its source's dtype and trailing shape"""
    return [torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for _, t, _ in entries]


def fill_table(struct, entries, new, P):
    """-> a ctypes array of `struct` {src, dst, row_words, kind}, one per entry; a tensor of no words has NULL pointers"""
    table = (struct * len(entries))()
    for slot, (kind, t, _), out in zip(table, entries, new):
        words = t.numel() // P
        slot.src, slot.dst, slot.row_words, slot.kind = (t.data_ptr() if words else None), \
            (out.data_ptr() if words else None), words, kind
    return table


def hand_over(pc, entries, new):
    """Gives every new tensor to its entry's destination, as _prune_optimizer / cat_tensors_to_optimizer
    (scene/gaussian_model.py:502-522, :570-590): the old key deleted, the SAME state dict under the new parameter,
    group["params"][0] and the model's attribute replaced; a group without state has only its parameter moved."""
    params = {}
    for (_, _, dest), out in zip(entries, new):
        if dest[0] == "param":
            _, group, attr, state = dest
            if state is not None:
                del pc.optimizer.state[group["params"][0]]
            p = nn.Parameter(out.requires_grad_(True))
            group["params"][0] = p
            if state is not None:
                pc.optimizer.state[p] = state
            setattr(pc, attr, p)
            params[id(group)] = p
        elif dest[0] == "state":
            dest[1][dest[2]] = out
        elif dest[0] == "grad":
            params[id(dest[1])].grad = out
        else:
            setattr(pc, dest[1], out)
