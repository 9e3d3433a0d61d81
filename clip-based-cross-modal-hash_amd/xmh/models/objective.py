"""The autograd bridge of the objectives that are ONE forward call and ONE gradient call of the library: HyP (dsph.py), DNPH, DIMCH
and UMoED.  ``Objective.apply(spec, consts, aux, *inputs)`` runs ``spec.loss`` and hands back the terms; its backward runs
``spec.grad`` for every input that needs a gradient.  A method supplies a ``Spec`` -- what differs between them -- and nothing else.
DCMHT (several calls per direction), TwDH (one call per modality over strided views) and MITH (its gradient entry takes one array
of pointers, its upstream is the whole vector, and its rolling buffer is saved as it is for autograd's version check) keep their own
functions."""
import collections

import torch

from .._lib import check, current_stream, ptr, workspace


def need_cuda(*tensors):
    """the losses' one device check: there is no CPU arithmetic to fall back to"""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("xmh losses need CUDA/HIP tensors (got %s); there is no CPU fallback" % t.device)


# loss, grad   the two entries (functions of xmh._lib.lib)
# pack         (consts, aux, ts) -> (dims, lead): the extents the workspace is sized by, and the C arguments up to the workspace
#              (gradient entry: up to the upstream pointer).  consts: the method's non-tensor arguments; aux: its tensors that take no
#              gradient (packed labels, DNPH's noises; None allowed); ts: the inputs as contiguous fp32
# ws_bytes     (*dims) -> bytes; 0 means out of range, and the bridge raises RuntimeError(bounds % dims)
# bounds       that message, a format of dims
# out_len      doubles the forward entry writes
# terms        how many of them are returned, as fp32 [terms] whose element 0 carries the gradient; 0: out[0] as a 0-dim tensor
# null_grads   whether the gradient entry takes NULL for a gradient nobody asked for (HyP's writes all three)
Spec = collections.namedtuple("Spec", "loss grad pack ws_bytes bounds out_len terms null_grads", defaults=(True,))


class Objective(torch.autograd.Function):

    @staticmethod
    def _args(spec, consts, aux, ts):
        dims, lead = spec.pack(consts, aux, ts)
        nbytes = spec.ws_bytes(*dims)
        if nbytes == 0:
            raise RuntimeError(spec.bounds % dims)
        return lead, workspace(nbytes, ts[0].device)

    @staticmethod
    def forward(ctx, spec, consts, aux, *inputs):
        ts = [t.detach().float().contiguous() for t in inputs]
        lead, ws = Objective._args(spec, consts, aux, ts)
        out = torch.empty(spec.out_len, dtype=torch.float64, device=ts[0].device)
        check(spec.loss(*lead, ptr(ws), ws.numel(), ptr(out), current_stream()), spec.loss.__name__)
        ctx.spec, ctx.consts, ctx.n_aux = spec, consts, len(aux)
        ctx.meta = [(t.shape, t.dtype) for t in inputs]
        ctx.save_for_backward(*aux, *ts)                  # a None among aux is saved and comes back as None
        return out[:spec.terms].float() if spec.terms else out[0].float()

    @staticmethod
    @torch.autograd.function.once_differentiable      # the gradient kernels are not themselves differentiable: fail loudly on double backward
    def backward(ctx, g):
        spec, saved = ctx.spec, ctx.saved_tensors
        aux, ts = saved[:ctx.n_aux], saved[ctx.n_aux:]
        lead, ws = Objective._args(spec, ctx.consts, aux, ts)
        up = g.detach().float()
        up = (up[:1] if up.dim() else up.reshape(1)).contiguous()      # only element 0 (the loss) carries a gradient
        need = ctx.needs_input_grad[3:]
        grads = [torch.empty_like(t) if nd or not spec.null_grads else None for t, nd in zip(ts, need)]
        check(spec.grad(*lead, ptr(up), *[ptr(t) for t in grads], 0, ptr(ws), ws.numel(), current_stream()), spec.grad.__name__)
        return (None, None, None, *[t.reshape(s).to(d) if nd else None for t, (s, d), nd in zip(grads, ctx.meta, need)])
