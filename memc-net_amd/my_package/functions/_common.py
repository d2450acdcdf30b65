"""Shared host-side plumbing of the operator Functions."""
import torch


def require_gpu(name, *tensors):
    """The reference's CPU branches raise NameError before reaching C (they never allocate `output`,
    FilterInterpolationLayer.py:23,32; FlowProjectionLayer.py:21-22,32); say so instead."""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "%s: CPU tensors are not supported -- there is no CPU path (the reference's own CPU "
                "branch is unrunnable); move the tensors to the GPU" % name)


def check(err, name):
    """The reference prints a non-zero error code and carries on with zero-filled results
    (FlowProjectionLayer.py:33-34); a drop-in that silently returns zeros hides real bugs, so raise."""
    if err != 0:
        raise RuntimeError("%s returned %d: shape/stride check failed or the launch failed" % (name, err))


def declined(err, name):
    """Return code 1 of a satellite library: the call is not covered and nothing was touched, so the caller takes its
    other route -- True.  0: False.  Anything else raises (check)."""
    if err == 1:
        return True
    check(err, name)
    return False


def f32c(t):
    """contiguous float32 view/copy (the reference caches `.contiguous()` copies for backward,
    FilterInterpolationLayer.py:14-16, and only ever sees torch.cuda.FloatTensor)."""
    if t.dtype != torch.float32:
        raise TypeError("expected a float32 tensor, got %s" % t.dtype)
    return t.contiguous()


# ---- the dtype rule of the operators (fp16 / bf16 next to float32) ----------------------------------------------------
LOWP = (torch.float16, torch.bfloat16)


def payload_dtype(*tensors):
    """The payload dtype of a call: torch.promote_types over its payload tensors (image / features, filter taps,
    occlusions).  float32 calls go exactly the old way; float16 / bfloat16 ones take libmemc_hip_lp.so where it has a
    kernel.  Anything else raises TypeError."""
    dt = tensors[0].dtype
    for t in tensors[1:]:
        dt = torch.promote_types(dt, t.dtype)
    if dt != torch.float32 and dt not in LOWP:
        raise TypeError("expected float32, float16 or bfloat16 tensors, got %s" % dt)
    return dt


def cast(t, dtype):
    """`t` in `dtype` (through autograd: the gradient comes back in t's own dtype); no copy when it already is."""
    return t if t.dtype == dtype else t.to(dtype)


def cast_like(grads, inputs):
    """each gradient in its input's dtype; a None stays None"""
    return tuple(None if g is None else cast(g, t.dtype) for g, t in zip(grads, inputs))


def flow_dtype(flow, payload):
    """A flow is decoded in the half kernels when it is float32 or of the payload dtype; any other dtype is cast to
    float32.  float32 payloads take float32 flows."""
    return flow.dtype if payload in LOWP and flow.dtype in (torch.float32, payload) else torch.float32


def host_widened(apply, like, *args):
    """The operators and calls without half kernels: the FlowProjection and DepthFlowProjection forwards, FlowProjection and
    DepthFlowProjection where their layers' `native_half_backward` is off (their backward passes have half kernels,
    FlowProjectionLayer.py and DepthFlowProjectionLayer.py), DepthFlowProjection with a float32 tensor beside a half one,
    Interpolation / InterpolationCh where their layers' `native_half` is off or the image is
    float32 beside a half flow (a half image has half kernels, InterpolationLayer.py; a backward they do not cover widens the
    saved tensors by itself, not through here): float16 / bfloat16 tensors among `args` are widened to float32 on the host,
    `apply` (the float32 Function) runs, and the result comes back in `like`'s dtype -- so that a cast model's concatenations
    and convolutions see one dtype.  Gradients flow back through the casts, each in its input's dtype.  Float32 arguments pass
    untouched."""
    out = apply(*(cast(a, torch.float32) if isinstance(a, torch.Tensor) and a.dtype in LOWP else a for a in args))
    return cast(out, like.dtype) if like.dtype in LOWP else out
