"""The table of the argument-contract tests ("The argument contract"): one row per public
wrapper of ``fourier_feature_nets_amd/ops.py`` and ``mlp_engine.py`` that reaches the library, with a
builder of ONE valid call at the smallest shapes.  tests/test_wrapper_refusals_cpu.py derives the
mutated calls from the rows and holds every wrapper to the rule: a mis-shaped tensor is a
``ValueError`` that names the wrapper and the argument, before anything reaches the library and
without reading a tensor's values.  tests/test_wrapper_refusals_gpu.py repeats a few of them on
device tensors.

The subjects come from the code (``subjects``), not from this table: a wrapper without a row fails
the CPU test.  Importing this module needs neither a GPU nor the library.

Sizes that play different roles are pairwise different small numbers, so that a check that compares
the wrong pair of dimensions cannot pass by coincidence."""

import ast
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "fourier_feature_nets_amd")
MODULES = ("ops", "mlp_engine")

# rays of a batch, samples per ray, rays of the sampler's table, leaves, interior nodes, channels,
# cameras, image height and width, focus samples, points, vertices, triangles, texels, grid side
R, S, T, L, NODES, C, CAMS, H, W, NF, P, V, F, TEX, G = 5, 3, 11, 7, 2, 4, 2, 6, 9, 2, 13, 10, 8, 17, 3
DEPTH = 3


# ------------------------------------------------------------------------------------ subjects
def _functions(tree):
    """qualified name -> FunctionDef of a module's functions and methods."""
    found = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            found[node.name] = node
        elif isinstance(node, ast.ClassDef):
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef):
                    found[node.name + "." + sub.name] = sub
    return found


def _launches(fn):
    """Does the body hold ``_call(...)`` or ``_lib.call(...)``?"""
    for node in ast.walk(fn):
        if isinstance(node, ast.Call):
            f = node.func
            if isinstance(f, ast.Name) and f.id == "_call":
                return True
            if (isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name)
                    and f.value.id == "_lib"):
                return True
    return False


def _callees(name, fn, functions):
    """The functions of the same module that ``fn`` calls: plain names, and ``self.x`` in a method."""
    owner = name.rsplit(".", 1)[0] if "." in name else None
    out = set()
    for node in ast.walk(fn):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Name) and f.id in functions:
            out.add(f.id)
        elif (owner and isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name)
              and f.value.id == "self" and owner + "." + f.attr in functions):
            out.add(owner + "." + f.attr)
    return out


def _private(name):
    return any(part.startswith("_") for part in name.split("."))


def module_subjects(source):
    """The public functions and methods of one module's source whose body reaches the library,
    directly or through private helpers of the same module."""
    functions = _functions(ast.parse(source))
    reach = {name for name, fn in functions.items() if _launches(fn)}
    grew = True
    while grew:
        grew = False
        for name, fn in functions.items():
            if name in reach:
                continue
            if any(c in reach and _private(c) for c in _callees(name, fn, functions)):
                reach.add(name)
                grew = True
    return sorted(name for name in reach if not _private(name))


def subjects():
    """Every subject of the contract, ``ops`` functions by their name and ``mlp_engine`` methods as
    ``Class.method``."""
    names = []
    for module in MODULES:
        with open(os.path.join(PACKAGE, module + ".py")) as f:
            names += module_subjects(f.read())
    assert len(names) == len(set(names))
    return names


# ------------------------------------------------------------------------------------ the table
class Row:
    """``build(make)`` -> the keyword arguments of one valid call; ``make(shape, dtype, fill)``
    makes a tensor (``fill`` only matters for ``marked`` rows).

    ``marked``: the wrapper's EXISTING checks read values (a finite ``proj``, the read-backs of
    ``mesh_sample`` and ``octree_refine``): the row gets CPU tensors filled as the builder asks.
    ``ints``: ``name -> (low, high)``, the bounds include/ffn_hip.h documents (``None`` = unbounded).
    ``optional``: parameters that may be ``None`` although the signature gives no default.
    ``who``: the regular expression of the wrapper's name in its messages (existing checks name
    themselves in their own words).  ``blames``: ``parameter -> names``, other words a refusal of
    that parameter's mutations may use instead of its name (an existing message, or a partner whose
    extent is defined by this parameter).  ``gpu_only``: a method that a planning-only program (all
    a machine without a GPU can build) does not have; the GPU test runs its row.  ``defines``: ``parameter -> mutation kinds`` that only
    change a size which this tensor alone states (the samples per ray of ``t_values``, the N of
    ``positions``): the mutated call is a valid call of another size and MUST pass every check.
    Such an entry grants no slack on an extent: the wrapper passes the new size to the entry point
    as a count, so every buffer keeps the extent the call states.  A size that another argument
    also bounds is no entry (a ``rows`` one column narrower than ``sigma_offset`` allows)."""

    def __init__(self, subject, build, ints, marked, optional, who, blames, defines=None,
                 gpu_only=False):
        self.gpu_only = bool(gpu_only)
        self.subject, self.build = subject, build
        self.ints, self.marked, self.optional = dict(ints or {}), bool(marked), tuple(optional)
        self.who = who or re.escape(subject.rsplit(".", 1)[-1] if subject.startswith("MlpProgram")
                                    else subject)
        self.blames = {k: (v,) if isinstance(v, str) else tuple(v)
                       for k, v in (blames or {}).items()}
        self.defines = {k: tuple(v.split()) for k, v in (defines or {}).items()}

    def target(self, kwargs):
        """(callable, its keyword arguments) of the valid call."""
        kwargs = dict(kwargs)
        if "." in self.subject:
            owner = kwargs.pop("_self")
            return getattr(owner, self.subject.rsplit(".", 1)[1]), kwargs
        from fourier_feature_nets_amd import ops
        return getattr(ops, self.subject), kwargs


ROWS = {}


def row(subject, ints=None, marked=False, optional=(), who=None, blames=None, defines=None,
        gpu_only=False):
    def add(build):
        assert subject not in ROWS, subject
        ROWS[subject] = Row(subject, build, ints, marked, optional, who, blames, defines, gpu_only)
        return build
    return add


def _torch():
    import torch
    return torch


def f32():
    return _torch().float32


def i64():
    return _torch().int64


def i32():
    return _torch().int32


def u8():
    return _torch().uint8


# ------------------------------------------------------------------------------------ the harness
class ReachedLibrary(Exception):
    """The hook that stands in for ``_lib.call``: it records the entry point and raises."""


class Hook:
    def __init__(self):
        self.seen = []

    def __call__(self, name, *args):
        self.seen.append(name)
        raise ReachedLibrary(name)

    def install(self, monkeypatch):
        from fourier_feature_nets_amd import _lib
        monkeypatch.setattr(_lib, "call", self)
        return self


def factory(device, filled):
    """``make(shape, dtype, fill)``: ``meta`` tensors carry no values (``fill`` is ignored), CPU and
    GPU tensors hold ``fill`` (a number, or a function of the shape -> nested lists / a tensor)."""
    torch = _torch()

    def make(shape, dtype=None, fill=0):
        dtype = dtype or torch.float32
        if not filled:
            return torch.empty(tuple(shape), dtype=dtype, device=device)
        if callable(fill):
            return torch.as_tensor(fill(tuple(shape)), dtype=dtype).reshape(tuple(shape)).to(device)
        return torch.full(tuple(shape), fill, dtype=dtype, device=device)
    return make


def _resized(t, shape):
    """A tensor like ``t`` of another shape: the leading block of ``t`` where it fits, zeros else."""
    torch = _torch()
    out = torch.zeros(shape, dtype=t.dtype, device=t.device)
    if t.device.type != "meta" and t.dim() == len(shape):
        window = tuple(slice(0, min(a, b)) for a, b in zip(t.shape, shape))
        out[window] = t[window]
    return out


def reads_shape(fn, name):
    """Does the wrapper, or a private helper of its module (or class) that it calls, read
    ``name.shape``?  (A helper is handed the argument under its own name: the checks of
    ``MlpProgram.forward`` read ``positions.shape`` inside ``_want_samples``.)"""
    import sys
    source = inspect.getsource(fn)
    module = sys.modules[fn.__module__]
    owner = getattr(fn, "__self__", None)
    for helper in set(re.findall(r"\b(?:self\.)?(_[A-Za-z]\w*)\(", source)):
        found = getattr(type(owner), helper, None) if owner is not None else None
        found = found or getattr(module, helper, None)
        if inspect.isfunction(found) and found.__module__ == fn.__module__:
            source += inspect.getsource(found)
    return re.search(r"\b%s\.shape\b" % re.escape(name), source) is not None


def mutations(row, fn, kwargs):
    """-> [(parameter, kind, mutated keyword arguments)] of one valid call: per tensor argument one
    row fewer, one more and one fewer in the last dimension, one dimension more where the wrapper
    reads its ``.shape``, ``None`` where the argument is required; per bounded integer the first
    value outside each bound."""
    torch = _torch()
    required = {name for name, p in inspect.signature(fn).parameters.items()
                if p.default is inspect.Parameter.empty} - set(row.optional)
    out = []

    def add(name, kind, value):
        changed = dict(kwargs)
        changed[name] = value
        out.append((name, kind, changed))

    for name, t in kwargs.items():
        if not torch.is_tensor(t):
            continue
        shape = tuple(t.shape)
        if t.dim() == 0:
            add(name, "last+1", _resized(t, (2,)))
            add(name, "last-1", _resized(t, (0,)))
        else:
            if t.dim() > 1 and shape[0] > 0:
                add(name, "row-1", _resized(t, (shape[0] - 1,) + shape[1:]))
            add(name, "last+1", _resized(t, shape[:-1] + (shape[-1] + 1,)))
            if shape[-1] > 0:
                add(name, "last-1", _resized(t, shape[:-1] + (shape[-1] - 1,)))
            if reads_shape(fn, name):
                add(name, "unsqueeze", t.unsqueeze(0))
        if name in required:
            add(name, "None", None)
    for name, (low, high) in row.ints.items():
        assert name in kwargs, "%s: no integer %s in the valid call" % (row.subject, name)
        if low is not None:
            add(name, "below", low - 1)
        if high is not None:
            add(name, "above", high + 1)
    return out


REFUSED, ACCEPTED_CALL, REACHED, READ_VALUES, BROKE = "refused", "accepted", "reached", "read", "broke"


def outcome(fn, kwargs, hook):
    """Runs one call under the hook -> (what happened, the exception or None).  ``accepted``: every
    check passed -- the call ended in ``_dev``'s "must live on the GPU", or returned without a
    launch.  ``reached``: the hook was called.  ``read``: a check wanted a tensor's values, which
    ``meta`` tensors do not have."""
    before = len(hook.seen)
    try:
        fn(**kwargs)
    except ReachedLibrary as e:
        return REACHED, e
    except (ValueError, TypeError) as e:
        kind = REFUSED
        if "meta" in str(e).lower():
            kind = READ_VALUES
        return (REACHED if len(hook.seen) > before else kind), e
    except NotImplementedError as e:            # torch: "Cannot copy out of meta tensor; no data!"
        return (READ_VALUES if "meta" in str(e).lower() else BROKE), e
    except RuntimeError as e:
        if len(hook.seen) > before:
            return REACHED, e
        if "must live on the GPU" in str(e) or re.search(r"lives on \w+ but the model is on", str(e)):
            return ACCEPTED_CALL, e                 # the device refusals that follow the checks
        return (READ_VALUES if "meta" in str(e).lower() else BROKE), e
    except Exception as e:                      # an IndexError or AttributeError is no refusal
        return BROKE, e
    return (REACHED if len(hook.seen) > before else ACCEPTED_CALL), None


def names_it(row, name, error):
    """Does the refusal name the wrapper and the argument?"""
    text = str(error)
    words = (name,) + row.blames.get(name, ())
    return (re.search(row.who, text) is not None
            and any(re.search(r"(?<![A-Za-z0-9])%s(?![A-Za-z0-9])" % re.escape(w), text)
                    for w in words))


# ------------------------------------------------------------------------------------ K1 .. K11
BOX = dict(box_lo=(-1.0, -1.0, -1.0), box_hi=(1.0, 1.0, 1.0))


@row("raygen_nearfar", ints=dict(width=(1, None), height=(1, None)), blames=dict(unproj="cam_pos"))
def _raygen(make):
    return dict(unproj=make((CAMS, 4, 4)), cam_pos=make((CAMS, 3)), width=W, height=H,
                points=make((W * H, 2)), **BOX)


@row("sample_t", ints=dict(count=(1, None)), optional=("noise", "anneal"),
     blames=dict(ray_index=("noise", "out")), defines=dict(near_far="last+1 last-1"))
def _sample_t(make):
    return dict(near_far=make((2, T)), ray_index=make((R,), i64()), count=S, unit=make((S,)),
                noise=make((R, S)), anneal=0.5, out=make((R, S)))


@row("materialise_samples", blames=dict(starts="directions", t_values="ray_index"),
     defines=dict(t_values="last+1 last-1"))
def _materialise(make):
    return dict(starts=make((T, 3)), directions=make((T, 3)), ray_index=make((R,), i64()),
                t_values=make((R, S)))


@row("sample_materialise", ints=dict(count=(1, None)), optional=("noise", "anneal"),
     blames=dict(starts="directions", ray_index="noise"), defines=dict(near_far="last+1 last-1"))
def _sample_materialise(make):
    return dict(near_far=make((2, T)), starts=make((T, 3)), directions=make((T, 3)),
                ray_index=make((R,), i64()), count=S, unit=make((S,)), noise=make((R, S)),
                anneal=None)


@row("cdf_build", blames=dict(t_probe="opacity"))
def _cdf_build(make):
    return dict(t_probe=make((R, S)), opacity=make((R, S)))


@row("cdf_build_logits", blames=dict(t_probe="logits"))
def _cdf_build_logits(make):
    return dict(t_probe=make((R, S)), logits=make((R * S, 4)))


@row("focus_sample_merge", ints=dict(n_focus=(1, S)),
     blames=dict(t_io=("ray_index", "n_focus", "cdfs", "u"), near_far=("cdfs",)),
     defines=dict(near_far="last-1", t_io="last+1 last-1"))
def _focus_merge(make):
    return dict(near_far=make((2, T)), cdfs=make((T, NF - 1)), ray_index=make((R,), i64()),
                u=make((R, NF)), unit_focus=make((NF,)), t_io=make((R, S)), n_focus=NF)


@row("to_image", ints=dict(width=(1, None), height=(1, None)),
     blames=dict(pixel_index=("pixel ids",), colors=("colours",)))
def _to_image(make):
    return dict(colors=make((R, 3)), pixel_index=make((R,), i64()), width=W, height=H)


@row("ycrcb_to_rgb_u8", defines=dict(image="row-1 unsqueeze"))
def _ycrcb(make):
    return dict(image=make((H, W, 3), u8()))


@row("fourier_encode", optional=("b", "a"), blames=dict(b=("a",)), defines=dict(x="row-1"))
def _fourier_encode(make):
    return dict(x=make((P, 3)), b=make((3, C)), a=make((C,)), scale=1.0, include_input=True)


@row("composite_fwd", blames=dict(t="logits"))
def _composite_fwd(make):
    return dict(logits=make((R, S, 4)), t=make((R, S)), include_depth=True,
                nan_flag=make((1,), i32()))


@row("blend_weights", blames=dict(t="sigma"))
def _blend_weights(make):
    return dict(t=make((R, S)), sigma=make((R, S)))


@row("blend_weights_bwd", blames=dict(t="sigma"))
def _blend_weights_bwd(make):
    return dict(t=make((R, S)), sigma=make((R, S)), d_weights=make((R, S)), want_dt=True)


@row("composite_bwd", blames=dict(t="logits"))
def _composite_bwd(make):
    return dict(logits=make((R, S, 4)), t=make((R, S)), d_color=make((R, 3)), d_alpha=make((R,)))


def _ground_truth(make):
    return dict(gt_colors=make((T, 3)), gt_alphas=make((T,)), ray_index=make((R,), i64()),
                color_scale=1.0 / (3 * R), alpha_scale=0.1 / R)


@row("mse_loss", optional=("gt_alphas",), blames=dict(color=("alpha",), gt_colors=("gt_alphas",)))
def _mse_loss(make):
    return dict(color=make((R, 3)), alpha=make((R,)), sums_out=make((2,)), **_ground_truth(make))


@row("composite_train", optional=("gt_alphas",),
     blames=dict(t="logits", gt_colors=("gt_alphas",)))
def _composite_train(make):
    return dict(logits=make((R, S, 4)), t=make((R, S)), nan_flag=make((1,), i32()),
                **_ground_truth(make))


@row("loss_from_partials", defines=dict(partials="row-1"))
def _loss_from_partials(make):
    return dict(partials=make((C, 2)), rays=R, alpha_weight=0.1, sums_out=make((2,)))


@row("loss_value")
def _loss_value(make):
    return dict(sums=make((2,)), rays=R, alpha_weight=0.1)


def _regression(make, c=3, d_logits=True):
    out = dict(logits=make((P, 4)), target=make((P, c)), partials=make((1,)))
    if d_logits:
        out["d_logits"] = make((P, 4))
    return out


@row("regression_train", blames=dict(target=("logits",)), defines=dict(target="last+1 last-1"))
def _regression_train(make):
    return _regression(make)


@row("regression_mse_train", blames=dict(target=("logits",)), defines=dict(target="last+1 last-1"))
def _regression_mse_train(make):
    return _regression(make)


@row("regression_mse_eval", blames=dict(target=("logits",)), defines=dict(target="last+1 last-1"))
def _regression_mse_eval(make):
    return _regression(make, d_logits=False)


@row("regression_eval", ints=dict(c=(1, 4)), optional=("target", "partials"),
     blames=dict(logits=("target",), target=("logits",)))
def _regression_eval(make):
    return dict(c=3, image=make((P, 3), u8()), **_regression(make, d_logits=False))


@row("regression_loss", defines=dict(partials="last+1 last-1"))
def _regression_loss(make):
    return dict(partials=make((C,)), count=P * 3, sse_out=make(()), loss_out=make(()))


@row("regression_mse_loss", defines=dict(partials="last+1 last-1"))
def _regression_mse_loss(make):
    return dict(partials=make((C,)), count=P * 3, sse_out=make(()), loss_out=make(()))


@row("clip_adam", ints=dict(step=(1, None)), blames=dict(params=("grads",)))
def _clip_adam(make):
    n = 1031                                            # two reduction blocks of 1024, ragged
    return dict(params=make((n,)), grads=make((n,)), exp_avg=make((n,)), exp_avg_sq=make((n,)),
                step=1, lr=1e-3, scratch=make((2,)), norm_out=make((1,)))


@row("occupancy_build", ints=dict(resolution=(1, None)))
def _occupancy_build(make):
    return dict(logits=make((G ** 3, 4)), resolution=G, sigma_threshold=0.5, dilate=True)


@row("occupancy_compact", ints=dict(resolution=(1, None)), optional=("views",),
     blames=dict(positions=("views",)))
def _occupancy_compact(make):
    return dict(positions=make((P, 3)), views=make((P, 3)), box_min=(-1.0,) * 3,
                box_size=(2.0,) * 3, resolution=G, bits=make((1,), i32()))


@row("occupancy_from_octree", ints=dict(resolution=(1, 1024)), blames=dict(leaf_index=("rows",)))
def _occupancy_from_octree(make):
    return dict(leaf_index=make((L,), i64()), scale=1.0, center=(0.0,) * 3, box_min=(-1.0,) * 3,
                box_size=(2.0,) * 3, resolution=G, rows=make((L, C)), stride=C, sigma_offset=3,
                sigma_threshold=0.5, dilate=1, out=make((1,), i32()))


@row("scatter_logits", ints=dict(n=(R, None)), blames=dict(packed=("index",)))
def _scatter_logits(make):
    return dict(packed=make((R, 4)), index=make((R,), i32()), n=P)


@row("gather_logits", defines=dict(index="last+1 last-1"))
def _gather_logits(make):
    return dict(full=make((P, 4)), index=make((R,), i32()))


@row("voxels_forward", ints=dict(side=(1, None)), defines=dict(positions="row-1"))
def _voxels_forward(make):
    return dict(volume=make((4, G, G, G)), bias=make((4,)), positions=make((P, 3)), side=G,
                scale=1.0)


@row("voxels_backward", ints=dict(side=(1, 1024)), blames=dict(positions=("d_logits",)))
def _voxels_backward(make):
    from fourier_feature_nets_amd import ops
    words = (ops.voxels_backward_workspace_bytes(P, G) + 3) // 4
    return dict(positions=make((P, 3)), d_logits=make((P, 4)), side=G, scale=1.0,
                workspace=make((words,)), d_volume=make((4, G, G, G)), d_bias=make((4,)))


# ------------------------------------------------------------------------------------ octrees
def _walk(make, n=R):
    return dict(starts=make((n, 3)), directions=make((n, 3)), scale=1.0, depth=DEPTH,
                node_index=make((NODES,), i64()), leaf_index=make((L,), i64(), _leaf_ids))


def _leaf_ids(shape):
    return list(range(1, 1 + shape[0]))                 # level-1 ids, sorted


WALK = dict(ints=dict(depth=(1, 11)),
            defines=dict(node_index="last+1 last-1", leaf_index="last+1 last-1"))
WALK_LEAVES = dict(ints=dict(depth=(1, 11)), defines=dict(node_index="last+1 last-1"))
WALK_BLAMES = dict(starts=("directions",), leaf_index=("leaf_data", "leaf_rows", "rows", "out",
                                                       "d_leaf_data", "d_leaf_rows", "leaves"))


@row("octree_surface_points", blames=dict(alpha=("color", "depth")),
     defines=dict(color="last+1 last-1"))
def _surface_points(make):
    return dict(alpha=make((P,)), depth=make((P,)), starts=make((P, 3)), directions=make((P, 3)),
                threshold=0.5, color=make((P, C)))


@row("octree_path_codes", defines=dict(positions="row-1"))
def _path_codes(make):
    return dict(positions=make((P, 3)), center=(0.0,) * 3, scale=1.0, depth=DEPTH)


@row("octree_structure", blames=dict(sorted_codes=("perm",)))
def _structure(make):
    return dict(sorted_codes=make((P,), i32()), perm=make((P,), i64()), depth=DEPTH,
                min_leaf_size=1)


@row("octree_interior_nodes", defines=dict(leaf_ids="last+1 last-1"))
def _interior_nodes(make):
    return dict(leaf_ids=make((L,), i64()), depth=DEPTH)


@row("octree_leaf_means", blames=dict(data=("perm",), leaf_start=("leaf_count",)),
     defines=dict(data="last+1 last-1"))
def _leaf_means(make):
    return dict(data=make((P, C)), perm=make((P,), i64()), leaf_start=make((L,), i64()),
                leaf_count=make((L,), i32()))


@row("octree_query", defines=dict(positions="row-1", node_index="last+1 last-1",
                                  leaf_index="last+1 last-1"))
def _query(make):
    return dict(positions=make((P, 3)), scale=1.0, node_index=make((NODES,), i64()),
                leaf_index=make((L,), i64()))


@row("octree_leaf_geometry", defines=dict(leaf_index="last+1 last-1"))
def _leaf_geometry(make):
    return dict(leaf_index=make((L,), i64()), scale=1.0)


@row("octree_neighbors", defines=dict(node_index="last+1 last-1", leaf_index="last+1 last-1"))
def _neighbors(make):
    return dict(node_index=make((NODES,), i64()), leaf_index=make((L,), i64()))


@row("octree_walk", who=r"octree[ _]walk", blames=WALK_BLAMES,
     ints=dict(depth=(1, 11), max_length=(2, None)), defines=WALK["defines"])
def _octree_walk(make):
    return dict(max_length=4, **_walk(make))


@row("octree_spans", who=r"octree walk", blames=WALK_BLAMES, **WALK)
def _octree_spans(make):
    return _walk(make)


@row("octree_first_hit", who=r"octree walk", blames=WALK_BLAMES, **WALK)
def _octree_first_hit(make):
    return _walk(make)


@row("octree_render", who=r"octree (walk|render)", blames=WALK_BLAMES, **WALK_LEAVES)
def _octree_render(make):
    return dict(leaf_data=make((L, 3)), want_hit=True, **_walk(make))


@row("octree_render_volume", who=r"octree (walk|render_volume)", blames=WALK_BLAMES, **WALK_LEAVES)
def _octree_render_volume(make):
    return dict(leaf_data=make((L, 4)), **_walk(make))


@row("octree_render_volume_sh", who=r"octree (walk|render_volume_sh|SH)", blames=WALK_BLAMES,
     ints=dict(depth=(1, 11), degree=(1, 2)), defines=WALK_LEAVES["defines"])
def _octree_render_volume_sh(make):
    return dict(leaf_rows=make((L, 16)), degree=1, **_walk(make))


@row("octree_sh_accumulate", who=r"octree (sh_accumulate|SH)", ints=dict(degree=(1, 2)),
     blames=dict(logits=("leaf_data",)))
def _sh_accumulate(make):
    return dict(logits=make((L, 4)), leaf_data=make((L, 13)), weights=[1.0] * 4, inv_views=0.5,
                degree=1)


def _volume_grads(make):
    return dict(d_color=make((R, 3)), d_alpha=make((R,)), dist_scale=0.5,
                ray_distortion=make((R,)))


BACKWARD_BLAMES = dict(WALK_BLAMES, d_color=("d_alpha",), starts=("directions", "d_color"))


@row("octree_render_volume_backward", who=r"octree (walk|render_volume_backward)",
     blames=BACKWARD_BLAMES, **WALK_LEAVES)
def _render_volume_backward(make):
    return dict(leaf_data=make((L, 4)), d_leaf_data=make((L, 4)), **_volume_grads(make),
                **_walk(make))


@row("octree_render_volume_sh_backward", who=r"octree (walk|render_volume_sh_backward|SH)",
     blames=BACKWARD_BLAMES, ints=dict(depth=(1, 11), degree=(1, 2)),
     defines=WALK_LEAVES["defines"])
def _render_volume_sh_backward(make):
    return dict(leaf_rows=make((L, 16)), degree=1, d_leaf_rows=make((L, 16)),
                **_volume_grads(make), **_walk(make))


@row("octree_project", who=r"octree project", defines=dict(leaf_data="row-1"))
def _project(make):
    return dict(leaf_data=make((L, 4)))


@row("octree_project_sh", who=r"octree (project_sh|SH)", ints=dict(degree=(1, 2)),
     defines=dict(leaf_rows="row-1"))
def _project_sh(make):
    return dict(leaf_rows=make((L, 16)), degree=1)


@row("octree_tv", who=r"octree tv", blames=dict(rows=("plan",)))
def _octree_tv(make):
    from fourier_feature_nets_amd import ops
    edges = 3
    plan = ops.OctreeTVPlan(L, make((edges,), i32()), make((edges,), i32()),
                            make((2 * edges,), i32()), make((2 * edges,), i32()),
                            make((L,), i32()), make((L,), i32()), make((L,), i32()), 2)
    return dict(rows=make((L, 4)), plan=plan, weights=[1.0] * 4, eps=1e-3, d_rows=make((L, 4)),
                accumulate=True)


@row("octree_bake", who=r"octree bake", defines=dict(logits="row-1"))
def _bake(make):
    return dict(logits=make((L, 4)))


@row("octree_cell_centers", ints=dict(depth=(1, 11), count=(0, 8 ** (DEPTH - 1)),
                                      first_code=(0, 8 ** (DEPTH - 1) - P)))
def _cell_centers(make):
    return dict(first_code=0, count=P, center=(0.0,) * 3, scale=1.0, depth=DEPTH,
                device=make((1,)).device)


@row("octree_density_select", who=r"octree density select", ints=dict(depth=(1, 11)),
     defines=dict(logits="row-1"))
def _density_select(make):
    return dict(logits=make((P, 4)), first_code=0, tau=0.1, side=0.5, depth=DEPTH)


@row("octree_merge_level", who=r"octree merge level", ints=dict(depth=(2, 11), level=(1, DEPTH - 1)),
     blames=dict(codes=("levels",)))
def _merge_level(make):
    return dict(codes=make((P,), i32()), levels=make((P,), i32()), data=make((P, 4)), level=1,
                depth=DEPTH, rgb_tol=0.1, sigma_tol=0.1)


def _density_rows(make):
    return dict(rows=make((L, C)), stride=C, sigma_offset=3)


@row("octree_leaf_weights", who=r"octree (walk|leaf_weights)", blames=WALK_BLAMES, **WALK_LEAVES)
def _leaf_weights(make):
    return dict(out=make((L,)), **_density_rows(make), **_walk(make))


@row("octree_distortion", who=r"octree (walk|distortion)", blames=WALK_BLAMES, **WALK_LEAVES)
def _distortion(make):
    return dict(**_density_rows(make), **_walk(make))


@row("octree_focus_sample", who=r"octree focus_sample", ints=dict(depth=(1, 11)),
     blames=dict(starts=("directions",), directions=("starts",), near_far=("starts",),
                 leaf_index=("rows",), ray_index=("u",)),
     defines=dict(node_index="last+1 last-1", u="last+1 last-1"))
def _octree_focus_sample(make):
    walk = _walk(make, T)
    return dict(near_far=make((2, T)), ray_index=make((R,), i64()), center=(0.0,) * 3,
                u=make((R, NF)), t_uniform=make((R, S)), n_uniform=S, want_mass=True,
                **_density_rows(make), **walk)


@row("octree_refine", who=r"octree refine", marked=True, ints=dict(depth=(1, 11)),
     optional=("rows",), blames=dict(leaf_ids=("action", "rows")), defines=dict(rows="last+1 last-1"))
def _refine(make):
    return dict(leaf_ids=make((L,), i64(), _leaf_ids), rows=make((L, C)),
                action=make((L,), u8(), 1), depth=2)


# ------------------------------------------------------------------------------------ images
def _cameras(make):
    return dict(images_u8=make((CAMS, H, W, 4), u8(), 255), proj=make((CAMS, 3, 4), f32(), 1.0))


CARVE_INTS = dict(depth=(1, 11), alpha_u8=(1, 255), max_misses=(0, None), min_views=(0, None))


@row("octree_carve_select", marked=True, ints=dict(CARVE_INTS, count=(1, None)),
     blames=dict(images_u8=("mask_u8",)))
def _carve_select(make):
    return dict(mask_u8=make((CAMS, H, W), u8(), 1), first_code=0, count=P, center=(0.0,) * 3,
                scale=1.0, depth=DEPTH, alpha_u8=128, max_misses=0, min_views=1, sigma0=1.0,
                want_visited=True, **_cameras(make))


@row("octree_carve_box_level", marked=True, ints=dict(CARVE_INTS, level=(0, DEPTH - 1)),
     blames=dict(images_u8=("sat",)), defines=dict(candidates="last+1 last-1"))
def _carve_box_level(make):
    return dict(sat=make((CAMS, H + 1, W + 1), i32()), candidates=make((P,), i32()), level=1,
                center=(0.0,) * 3, scale=1.0, depth=DEPTH, alpha_u8=128, max_misses=0,
                min_views=1, sigma0=1.0, want_visited=True, **_cameras(make))


def _visible(make, fields):
    walk = _walk(make)
    return dict(leaf_centers=make((L, 3)), scale=1.0, depth=DEPTH, node_index=walk["node_index"],
                leaf_index=walk["leaf_index"], eyes=make((CAMS, 3), f32(), 2.0), alpha_u8=128,
                min_transmittance=0.0, out=make((L, fields), _torch().uint32),
                **_density_rows(make), **_cameras(make))


VISIBLE = dict(marked=True, ints=dict(depth=(1, 11), alpha_u8=(1, 255)),
               blames=dict(leaf_index=("leaf_centers",), images_u8=("proj",)),
               defines=dict(node_index="last+1 last-1"))


@row("octree_visible_votes", **VISIBLE)
def _visible_votes(make):
    return _visible(make, 4)


@row("octree_visible_moments", **VISIBLE)
def _visible_moments(make):
    return _visible(make, 8)


# ------------------------------------------------------------------------------------ meshes
@row("octree_mesh_solid", who=r"octree mesh", optional=("rows", "solid"),
     blames=dict(rows=("sigma_offset",)), defines=dict(rows="last+1"))
def _mesh_solid(make):
    return dict(rows=make((L, C)), sigma_offset=3, solid=make((L,), u8()), num_leaves=L, side=0.5,
                threshold=0.5, device=make((1,)).device)


@row("octree_mesh_candidates", who=r"octree mesh", ints=dict(count=(1, None), depth=(1, None)),
     blames=dict(leaf_index=("solid",)), defines=dict(node_index="last+1 last-1"))
def _mesh_candidates(make):
    return dict(node_index=make((NODES,), i64()), leaf_index=make((L,), i64()),
                solid=make((L,), u8()), cand_offsets=make((L + 1,), i64()), first=0, count=P,
                depth=DEPTH)


@row("octree_mesh_vertices", who=r"octree mesh", optional=("rows",),
     blames=dict(alpha=("rows",)), defines=dict(rows="last+1 last-1"))
def _mesh_vertices(make):
    return dict(keys=make((V,), i64()), masks=make((V,), u8()), samples=make((V, 8), i32()),
                alpha=make((L,)), rows=make((L, C)), color=(0, 1, 0), depth=DEPTH, scale=1.0,
                center=(0.0,) * 3, threshold=0.5, surface_nets=True)


@row("octree_mesh_faces", who=r"octree mesh", blames=dict(keys=("masks",)))
def _mesh_faces(make):
    return dict(keys=make((V,), i64()), masks=make((V,), u8()), depth=DEPTH)


def _mesh(make):
    return dict(vertices=make((V, 3)), triangles=make((F, 3), i32()))


def _proj():
    import numpy as np
    return np.eye(3, 4, dtype=np.float32)


FRAME_INTS = dict(width=(1, 16384), height=(1, 16384))


@row("mesh_sample", marked=True, blames=dict(vertices=("uvs",), triangles=("offsets",)),
     defines=dict(texture="row-1 last+1"))
def _mesh_sample(make):
    return dict(uvs=make((V, 2)), offsets=make((F + 1,), i32(), lambda shape: range(shape[0])),
                texture=make((H, W, 3), u8()), want_uvs=True, **_mesh(make))


@row("mesh_raster_setup", ints=FRAME_INTS, defines=dict(vertices="row-1", triangles="row-1"))
def _raster_setup(make):
    return dict(proj=_proj(), width=W, height=H, **_mesh(make))


@row("mesh_raster_draw", ints=dict(FRAME_INTS, count=(1, None), first=(0, None)),
     blames=dict(record=("offsets",)))
def _raster_draw(make):
    return dict(record=make((F, 16), i32()), offsets=make((F + 1,), i64()), first=0, count=P,
                width=W, height=H, zbuf=make((W * H,), i64()))


@row("mesh_raster_resolve", ints=FRAME_INTS, optional=("colors", "uvs", "texture"),
     blames=dict(vertices=("colors",), triangles=("record",)))
def _raster_resolve(make):
    return dict(zbuf=make((W * H,), i64()), record=make((F, 16), i32()), colors=make((V, 3)),
                uvs=None, texture=None, eye=(0.0, 0.0, 2.0), background=(0.0,) * 3, width=W,
                height=H, **_mesh(make))


@row("mesh_raster_face_sums", ints=FRAME_INTS, defines=dict(record="row-1"))
def _face_sums(make):
    return dict(record=make((F, 16), i32()), ids=make((W * H,), i32()), d_color=make((W * H, 3)),
                width=W, height=H)


@row("mesh_vertex_gather", blames=dict(face_sums=("corner_order",), vertex_starts=("grad",)))
def _vertex_gather(make):
    return dict(face_sums=make((F, 12)), corner_order=make((3 * F,), i32()),
                vertex_starts=make((V + 1,), i32()), grad=make((V, 3)), weight=make((V,)),
                accumulate=True)


@row("mesh_texture_taps", ints=dict(FRAME_INTS, tex_height=(1, None), tex_width=(1, None)),
     blames=dict(triangles=("record",), tex_height=("texture",), tex_width=("texture",)),
     defines=dict(uvs="row-1"))
def _texture_taps(make):
    return dict(record=make((F, 16), i32()), ids=make((W * H,), i32()),
                triangles=make((F, 3), i32()), uvs=make((V, 2)), tex_height=4, tex_width=5,
                width=W, height=H)


@row("mesh_texture_gather", blames=dict(tap_texel=("tap_weight",)), defines=dict(texture="row-1"))
def _texture_gather(make):
    return dict(tap_texel=make((W * H, 4), i32()), tap_weight=make((W * H, 4)),
                texture=make((TEX, 3)), background=(0.0,) * 3)


@row("mesh_texture_grad", ints=dict(num_texels=(1, None)),
     blames=dict(tap_weight=("sorted_texels",)))
def _texture_grad(make):
    return dict(sorted_texels=make((4 * W * H,), i32()), tap_order=make((4 * W * H,), i32()),
                tap_weight=make((W * H, 4)), d_color=make((W * H, 3)), num_texels=TEX,
                grad=make((TEX, 3)), weight=make((TEX,)), accumulate=True)


def _aa_frame(make):
    return dict(record=make((F, 16), i32()), zbuf=make((W * H,), i64()),
                ids=make((W * H,), i32()), opposite=make((3 * F,), i32()), vertices=make((V, 3)),
                proj=_proj(), color=make((W * H, 3)), alpha=make((W * H,)), width=W, height=H)


@row("mesh_aa_forward", ints=FRAME_INTS, blames=dict(record=("opposite",)),
     defines=dict(vertices="row-1"))
def _aa_forward(make):
    return _aa_frame(make)


@row("mesh_aa_backward", ints=FRAME_INTS, blames=dict(record=("opposite",)),
     defines=dict(vertices="row-1"))
def _aa_backward(make):
    return dict(triangles=make((F, 3), i32()), g_color=make((W * H, 3)), g_alpha=make((W * H,)),
                **_aa_frame(make))


@row("mesh_aa_vertex_grad", blames=dict(entry_grad=("sorted_vertex",), vertices=("grad",)))
def _aa_vertex_grad(make):
    return dict(sorted_vertex=make((4 * W * H,), i32()), order=make((4 * W * H,), i32()),
                entry_grad=make((4 * W * H, 2)), vertices=make((V, 3)), proj=_proj(),
                grad=make((V, 3)), accumulate=True)


@row("mesh_laplacian", blames=dict(values=("neighbor_starts",)),
     defines=dict(neighbors="last+1 last-1"))
def _laplacian(make):
    return dict(values=make((V, 3)), neighbor_starts=make((V + 1,), i32()),
                neighbors=make((P,), i32()), scale=1.0, out=make((V, 3)), accumulate=True)


# ------------------------------------------------------------------------------------ the MLP engine
def program(device):
    """A small NeRF's chain: two encodings (the second one of the view directions), a skip, fused
    heads.  On a machine without a GPU the program only plans (``planning_only``): its launch
    methods still run every check and end in ``_dev``'s refusal."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd.mlp_engine import MlpProgram
    torch = _torch()
    device = torch.device(device)
    model = ffn.NeRF(2, 32, 3, 4, 2, 2, [1], True)
    if device.type == "cuda":
        return model.to(device).program()
    enc, specs = model._chain(torch.device("cpu"))
    return MlpProgram(enc, specs, torch.device("cpu"), planning_only=True)


def _program_for(make):
    device = make((1,)).device
    return program("cuda" if device.type == "cuda" else "cpu")


@row("MlpProgram.forward", blames=dict(positions=("views", "saved")))
def _mlp_forward(make):
    prog = _program_for(make)
    return dict(_self=prog, positions=make((P, 3)), views=make((P, 3)),
                saved=make((prog.saved_floats(P),)))


@row("MlpProgram.forward16", blames=dict(positions=("views",)), gpu_only=True)
def _mlp_forward16(make):
    return dict(_self=_program_for(make), positions=make((P, 3)), views=make((P, 3)))


@row("MlpProgram.backward", blames=dict(positions=("views", "d_logits")))
def _mlp_backward(make):
    prog = _program_for(make)
    return dict(_self=prog, d_logits=make((P, 4)), positions=make((P, 3)), views=make((P, 3)),
                saved=make((prog.saved_floats(P),)), grads=make((prog.num_grad_floats,)))


@row("MlpProgram.render", who=r"MlpProgram\.render|^t_values must be",
     optional=("unit",),
     blames=dict(starts=("directions",), ray_index=("t_values",)),
     defines=dict(near_far="last-1", image="row-1 unsqueeze"))
def _mlp_render(make):
    return dict(_self=_program_for(make), starts=make((T, 3)), directions=make((T, 3)),
                near_far=make((2, T)), ray_index=make((R,), i64()), num_samples=S,
                unit=make((S,)), t_values=make((R, S)), want_depth=True,
                nan_flag=make((1,), i32()), image=make((H, W, 3), u8()))


@row("MlpProgram.focus_sample", ints=dict(n_focus=(1, S)),
     blames=dict(starts=("directions",), ray_index=("u",), t_io=("ray_index", "u", "n_focus")),
     defines=dict(near_far="last+1 last-1"))
def _mlp_focus_sample(make):
    return dict(_self=_program_for(make), starts=make((T, 3)), directions=make((T, 3)),
                near_far=make((2, T)), ray_index=make((R,), i64()), num_samples=S, n_focus=NF,
                unit_focus=make((NF,)), u=make((R, NF)), t_io=make((R, S)))


@row("MlpProgram.pack", gpu_only=True)
def _mlp_pack(make):
    return dict(_self=_program_for(make))


@row("MlpProgram.pack16", gpu_only=True)
def _mlp_pack16(make):
    return dict(_self=_program_for(make))


# ------------------------------------------------------------------------------------ exemptions
# Mutations that describe a LEGAL call: (subject, parameter, kind) -> the sentence of
# include/ffn_hip.h that allows it (the CPU test looks every sentence up in the header).
_WORKSPACE = "workspace: ffn_voxels_backward_workspace(N, S) bytes (-1 for an invalid shape)"
_PARTIALS = "partials: ffn_regression_blocks(n) floats, one sum((sigmoid - y)^2) per workgroup."
_WIDE3 = "leaf_data (num_leaves, channels) f32 with channels >= 3"
_WIDE4 = "(num_leaves, channels) f32 with channels >= 4"
_SAVED = "while the slabs in `saved` are addressed by the batch's block ids"
ACCEPTED = {
    ("sample_t", "out", "last+1"):
        "t_out (R, t_stride) -- the first `count` entries of each row are written",
    ("gather_logits", "full", "row-1"): "packed[i] = full[index[i]] for (.,4) rows",
    ("clip_adam", "scratch", "last+1"): "scratch (ceil(n/1024)) floats",
    ("voxels_backward", "workspace", "last+1"): _WORKSPACE,
    ("regression_train", "partials", "last+1"): _PARTIALS,
    ("regression_mse_train", "partials", "last+1"): _PARTIALS,
    ("regression_mse_eval", "partials", "last+1"): _PARTIALS,
    ("regression_eval", "partials", "last+1"): _PARTIALS,
    ("octree_render", "leaf_data", "last+1"): _WIDE3,
    ("octree_render_volume", "leaf_data", "last+1"): _WIDE4,
    ("octree_render_volume_backward", "leaf_data", "last+1"): _WIDE4,
    ("MlpProgram.forward", "saved", "last+1"): _SAVED,
    ("MlpProgram.backward", "saved", "last+1"): _SAVED,
    ("octree_focus_sample", "t_uniform", "last+1"):
        "uniform samples at t_uniform + r * uniform_stride (K2a's output)",
}

# Tensor parameters of which NO shape mutation is refused, because only their values decide what is
# read: (subject, parameter) -> (the reason, the header's sentence).  Validity by value is the
# caller's to keep ("The argument contract").
BY_VALUE_ONLY = {}
