"""Launch trace of the convolution family's and the pool / upsample family's host path: which C-ABI entry points `conv3d`,
`conv3d_cat`, `bayes_conv3d`, `conv3d_pair`, `conv_transpose3d`, `upsample_conv3d`, `max_pool3d`, `max_pool3d_skip` and `upsample3d`
call, in which order, with which geometries, integers and tensors, under
which `KernelTimer` tags, and which gradients their backward hands to autograd (a tensor, or None because a `GradSink` took it).

The recorder stands in for `ops._lib.lib()` while a case runs and forwards every call to the real library.  It writes down the entry
point's name, the fields of every geometry struct, every integer and float, and for every pointer a LABEL instead of its address:
`null`, the name the case gave the tensor that starts there (inputs, parameters, the supplied `dy` and `eps`, `sink:<param>` for the
view a `GradSink` writes into), `ws` for the per-stream workspace (its size too), `new` for anything allocated on the way.  The value
a workspace, statistics-block or support query returns is kept.  tests/golden/conv_host_trace.json holds the traces; it has names,
integers and labels only, so kernel work leaves it alone and it changes exactly when the host path launches something else.

The cases use the public API only, so this file runs unmodified on any commit: `python tests/test_conv_host_trace_gpu.py` rewrites
the golden from the checkout it runs in (do that on the commit BEFORE a change to the host path, and review the diff after one that
is meant to change a launch)."""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import resample_cases as rc  # noqa: E402
from mri_epilepsy_diagnosis_amd import ops, parallel  # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "conv_host_trace.json")
CL3D = torch.channels_last_3d
_QUERIES = ("workspace_bytes", "stats_blocks", "supported")


class Recorder:
    """`with Recorder(labels) as rec:` — see the module docstring.  labels: {tensor.data_ptr(): name}, open to additions."""

    def __init__(self, labels):
        self.labels, self.calls, self.ws = labels, [], {}
        self.real = ops._lib.lib()

    def __enter__(self):
        self.saved = (ops._lib.lib, ops._workspace)
        self.backwards = [(c, c.__dict__["backward"]) for c in vars(ops).values()
                          if isinstance(c, type) and issubclass(c, torch.autograd.Function) and "backward" in c.__dict__]
        for cls, fn in self.backwards:
            setattr(cls, "backward", staticmethod(self._backward(cls.__name__, fn.__func__)))
        ops._lib.lib = lambda: self
        ops._workspace = self._workspace
        self.timer = ops.KernelTimer()
        ops.set_timer(self.timer)
        return self

    def __exit__(self, *exc):
        ops._lib.lib, ops._workspace = self.saved
        ops.set_timer(None)
        for cls, fn in self.backwards:
            setattr(cls, "backward", fn)
        return False

    def _workspace(self, nbytes, device):
        ws = self.saved[1](nbytes, device)
        self.ws[ws.data_ptr()] = ws.numel()
        return ws

    def _backward(self, name, fn):
        def backward(ctx, *grads):
            out = fn(ctx, *grads)
            self.calls.append(["backward", name, ["None" if o is None else "tensor" for o in (out if isinstance(out, tuple) else (out,))]])
            return out
        return backward

    def _pointer(self, addr):
        if not addr:
            return "null"
        if addr in self.ws:
            return "ws"
        return self.labels.get(addr, "new")

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            rec, after_ws = [name], None
            for a in args:
                obj = getattr(a, "_obj", None)
                if isinstance(obj, ctypes.Structure):       # byref(geometry)
                    rec.append("%s(%s)" % (type(obj).__name__, ", ".join("%s=%s" % (f, getattr(obj, f)) for f, _ in obj._fields_)))
                elif a is None or isinstance(a, ctypes.c_void_p):
                    addr = None if a is None else a.value
                    rec.append(self._pointer(addr))
                    after_ws = self.ws[addr] if rec[-1] == "ws" else None
                    continue
                elif isinstance(a, bool):
                    rec.append(int(a))
                elif isinstance(a, (int, float)):
                    rec.append("ws" if after_ws is not None and a == after_ws else a)
                else:
                    rec.append(type(a).__name__)
                after_ws = None
            ret = fn(*args)
            if name.endswith(_QUERIES):
                rec.append({"returns": int(ret)})
            self.calls.append(rec)
            return ret
        return call

    def trace(self):
        return {"calls": self.calls, "tags": [r[0] for r in self.timer.records]}


# ------------------------------------------------------------------------------------------------------------------ cases
def _randn(seed, shape, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to("cuda", dtype)


def _act(seed, shape, grad=True, pad=0, dtype=torch.float32):
    """NDHWC activation of logical `shape`; pad > 0: the last channels of a buffer that is `pad` channels wider (a pitched slice)."""
    n, c = shape[:2]
    buf = _randn(seed, (n, c + pad) + tuple(shape[2:]), dtype).contiguous(memory_format=CL3D)
    x = buf.narrow(1, pad, c) if pad else buf
    return x.requires_grad_(grad)


def _param(seed, shape, grad=True, scale=0.2):
    return torch.nn.Parameter(_randn(seed, shape) * scale, requires_grad=grad)


class _Conv:
    """What `ops.conv3d_pair` reads of an nn.Conv3d."""

    def __init__(self, weight, bias, stride, padding):
        self.weight, self.bias, self.stride, self.padding, self.dilation = weight, bias, stride, padding, (1, 1, 1)


def _conv3d(xshape=(2, 16, 5, 6, 7), co=16, bias=True, x_pad=0, x_grad=True, w_grad=True, b_grad=True, autocast=False, **kw):
    def make():
        x = _act(1, xshape, x_grad, x_pad)
        w = _param(2, (co, xshape[1], 3, 3, 3), w_grad)
        b = _param(3, (co,), b_grad) if bias else None

        def fwd():
            with ops.autocast() if autocast else contextlib.nullcontext():
                return ops.conv3d(x, w, b, **kw)
        return {"x": x}, {"w": w, "b": b}, fwd
    return make


def _cat(n, sp, ca=32, cb=16, co=16, **kw):
    def make():
        xa, xb = _act(1, (n, ca) + sp), _act(2, (n, cb) + sp)
        w, b = _param(3, (co, ca + cb, 3, 3, 3)), _param(4, (co,))
        return {"xa": xa, "xb": xb}, {"w": w, "b": b}, lambda: ops.conv3d_cat(xa, xb, w, b, **kw)
    return make


def _bayes(stride=1, bias=True, training=True, eps=False, xshape=(2, 8, 5, 6, 7), co=8):
    def make():
        x = _act(1, xshape)
        mu, ls = _param(2, (co, xshape[1], 3, 3, 3)), torch.nn.Parameter(_randn(3, (co, xshape[1], 3, 3, 3)) * 0.1 - 3.0)
        mb, lb = (_param(4, (co,)), _param(5, (co,))) if bias else (None, None)
        tensors = {"x": x}
        if eps:
            out = tuple((i + 2 - 3) // stride + 1 for i in xshape[2:])
            tensors["eps"] = _act(6, (xshape[0], co) + out, False)
        return (tensors, {"mu": mu, "logsigma": ls, "mu_bias": mb, "logsigma_bias": lb},
                lambda: ops.bayes_conv3d(x, mu, ls, mb, lb, stride=stride, padding=1, training=training, eps=tensors.get("eps"))[0])
    return make


def _pair(k2, served=True):
    def make():
        x = _act(1, (2, 1, 8, 6, 5), False)
        c1 = _Conv(_param(2, (8, 1, 6, 1, 1)), _param(3, (8,)), (2, 1, 1), (2, 0, 0))
        c2 = _Conv(_param(4, (8, 8) + k2), _param(5, (8,)), (1, 1, 1), tuple(k // 2 for k in k2))
        assert ops.conv3d_pair_supported(x, c1, c2) == served
        return {"x": x}, {"w1": c1.weight, "b1": c1.bias, "w2": c2.weight, "b2": c2.bias}, lambda: ops.conv3d_pair(x, c1, c2)
    return make


def _transpose(stride=1, bias=True, output_padding=0, k=3):
    def make():
        x = _act(1, (2, 8, 3, 4, 5))
        w, b = _param(2, (8, 4, k, k, k)), _param(3, (4,)) if bias else None
        return {"x": x}, {"w": w, "b": b}, lambda: ops.conv_transpose3d(x, w, b, stride=stride, padding=1, output_padding=output_padding)
    return make


def _upconv(ci, co, sp, served=True):
    def make():
        x = _act(1, (2, ci) + sp)
        w, b = _param(2, (co, ci, 3, 1, 1)), _param(3, (co,))
        assert ops.upsample_conv3d_supported(x, w, 4, 1, (1, 0, 0), 1) == served
        return {"x": x}, {"w": w, "b": b}, lambda: ops.upsample_conv3d(x, 4, w, b, padding=(1, 0, 0))
    return make


def _smallest(rows):
    return min(rows, key=lambda r: r.c * r.sp[0] * r.sp[1] * r.sp[2])


def _pool():
    r = _smallest(rc.POOL)

    def make():
        x = _act(1, (rc.N, r.c) + r.sp)
        return {"x": x}, {}, lambda: ops.max_pool3d(x, r.k, r.s)
    return make


def _pool_skip():
    r = _smallest(rc.POOL_SKIP)

    def make():
        x = _act(1, (rc.N, r.c) + r.sp)
        return {"x": x}, {}, lambda: ops.max_pool3d_skip(x, 2)
    return make, r.pad


def _upsample(rows, out=False):
    r = _smallest(rows)

    def make():
        x = _act(1, (rc.N, r.c) + r.sp)
        tensors, dest = {"x": x}, None
        if out:     # the last r.c channels of a cat buffer twice as wide
            tensors["buf"] = ops.new_cat_buffer(rc.N, 2 * r.c, tuple(int(i * r.scale) for i in r.sp), x)
            dest = (tensors["buf"], r.c)
        return tensors, {}, lambda: ops.upsample3d(x, size=r.size, scale_factor=r.scale, mode=r.mode, align_corners=r.ac, out=dest)
    return make


_TRILINEAR_X2 = [r for r in rc.UP if r.mode == "trilinear" and r.scale == 2 and not r.ac]
_STATS_SERVED, _CAT_SERVED = (2, 16, 5, 9, 17), dict(n=32, sp=(5, 9, 17))      # (the smallest this library serves fused / split in fp32)
# name -> (make, options): dy_pad pitches the incoming gradient (of a node with two outputs: one pad each, None = that output is
# not used); sinks = "fresh" | "twice" | "suspended" attaches parallel.FlatParams
CASES = {
    "conv3d": (_conv3d(padding=1), {}),
    "conv3d_bn_stats_served": (_conv3d(_STATS_SERVED, padding=1, bn_stats=True), {}),
    "conv3d_bn_stats_unserved": (_conv3d(padding=1, bn_stats=True), {}),
    "conv3d_pitched_x_and_dy": (_conv3d(padding=1, x_pad=8), {"dy_pad": 8}),
    "conv3d_no_bias": (_conv3d(padding=1, bias=False), {}),
    "conv3d_bias_frozen": (_conv3d(padding=1, b_grad=False), {}),
    "conv3d_weight_frozen": (_conv3d(padding=1, w_grad=False), {}),
    "conv3d_x_no_grad": (_conv3d(padding=1, x_grad=False), {}),
    "conv3d_stride2_stuffed": (_conv3d((2, 8, 5, 6, 7), stride=2, padding=1), {}),
    "conv3d_stride2_autocast": (_conv3d((2, 8, 5, 6, 7), stride=2, padding=1, autocast=True), {}),
    "cat_served": (_cat(**_CAT_SERVED), {}),
    "cat_served_bn_stats": (_cat(bn_stats=True, **_CAT_SERVED), {}),
    "cat_refused": (_cat(2, (5, 6, 7), bn_stats=True), {}),
    "bayes_train": (_bayes(), {}),
    "bayes_eval": (_bayes(training=False), {}),
    "bayes_stride2": (_bayes(stride=2), {}),
    "bayes_no_bias": (_bayes(bias=False), {}),
    "bayes_eps": (_bayes(eps=True), {}),
    "bayes_stride2_no_bias_eps_eval": (_bayes(stride=2, bias=False, eps=True, training=False), {}),
    "pair_served": (_pair((1, 3, 1)), {}),
    "pair_refused": (_pair((3, 3, 3), served=False), {}),
    "transpose_bias": (_transpose(), {}),
    "transpose_stride2": (_transpose(stride=2, bias=False), {}),
    "transpose_output_padding": (_transpose(stride=2, output_padding=1), {}),
    "upconv_served": (_upconv(8, 1, (3, 4, 5)), {}),
    "upconv_refused": (_upconv(16, 8, (2, 3, 2), served=False), {}),
    "max_pool3d": (_pool(), {}),
    "max_pool3d_skip_both": (_pool_skip()[0], {"dy_pad": (0, 0)}),
    "max_pool3d_skip_pool_only": (_pool_skip()[0], {"dy_pad": (0, None)}),
    "max_pool3d_skip_skip_only": (_pool_skip()[0], {"dy_pad": (None, 0)}),
    "max_pool3d_skip_pitched_dskip": (_pool_skip()[0], {"dy_pad": (0, _pool_skip()[1])}),
    "upsample3d_nearest_x2": (_upsample([r for r in rc.UP if r.mode == "nearest" and r.scale == 2]), {}),
    "upsample3d_trilinear_x2": (_upsample(_TRILINEAR_X2), {}),
    "upsample3d_size": (_upsample([r for r in rc.UP if r.size is not None]), {}),
    "upsample3d_out_cat_buffer": (_upsample(_TRILINEAR_X2, out=True), {}),
}
for _name, _make in (("conv3d", _conv3d(padding=1)), ("cat", _cat(**_CAT_SERVED)), ("pair", _pair((1, 3, 1))), ("upconv", _upconv(8, 1, (3, 4, 5)))):
    for _mode in ("fresh", "twice", "suspended"):
        CASES["%s_sink_%s" % (_name, _mode)] = (_make, {"sinks": _mode})


def run_case(name):
    """(trace, {name: tensor}) of one case: the result, and the gradient of every input and parameter that takes one."""
    make, opt = CASES[name]
    sinks = opt.get("sinks")
    ops.release_workspaces()
    torch.manual_seed(0)           # (bayes_conv3d draws its noise from the default generator)
    tensors, params, fwd = make()
    params = {k: p for k, p in params.items() if p is not None}
    if sinks:
        flat = parallel.FlatParams(torch.nn.ParameterList(list(params.values())))      # (moves the parameters into its flat buffer)
        flat.zero_grad()
    labels = {t.data_ptr(): k for k, t in list(tensors.items()) + list(params.items())}
    if sinks:
        labels.update({p.grad.data_ptr(): "sink:" + k for k, p in params.items()})
    with Recorder(labels) as rec, ops.suspend_grad_sinks() if sinks == "suspended" else contextlib.nullcontext():
        ys = [fwd() for _ in range(2 if sinks == "twice" else 1)]
        if isinstance(ys[0], tuple):        # one node with two outputs: their gradients are "dy" and "dy1", each with its own pad
            ys = list(ys[0])
            dys = [None if pad is None else _act(9 + i, tuple(y.shape), False, pad, y.dtype) for i, (y, pad) in enumerate(zip(ys, opt["dy_pad"]))]
        else:
            dys = [_act(9, tuple(ys[0].shape), False, opt.get("dy_pad", 0), ys[0].dtype)] * len(ys)
        for i, dy in enumerate(dys):
            if dy is not None:
                labels.setdefault(dy.data_ptr(), "dy%d" % i if i else "dy")
        used = [(y, dy) for y, dy in zip(ys, dys) if dy is not None]
        if used[0][0].requires_grad:
            torch.autograd.backward([y for y, _ in used], [dy for _, dy in used])
        torch.cuda.synchronize()
        trace = rec.trace()
    out = {"y": ys[0].detach()}
    out.update({"d" + k: t.grad for k, t in list(tensors.items()) + list(params.items()) if t.grad is not None})
    return trace, out


def _golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_host_path_launches_what_the_golden_trace_records(name):
    trace, _ = run_case(name)
    want = _golden()[name]
    got = json.loads(json.dumps(trace))
    assert got["tags"] == want["tags"]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, "call %d differs" % i
    assert len(got["calls"]) == len(want["calls"])


def test_golden_has_exactly_the_cases():
    assert sorted(_golden()) == sorted(CASES)


if __name__ == "__main__":
    traces = {name: run_case(name)[0] for name in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN_FILE, "w") as f:       # one call per line
        f.write("{\n" + ",\n".join('%s: {"tags": %s, "calls": [\n%s\n]}' % (json.dumps(k), json.dumps(t["tags"]), ",\n".join(json.dumps(c) for c in t["calls"]))
                                   for k, t in sorted(traces.items())) + "\n}\n")
    print("wrote %d traces, %d calls" % (len(traces), sum(len(t["calls"]) for t in traces.values())))
