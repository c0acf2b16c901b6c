"""The Sinkhorn coarse matcher stated in torch, dtype-generic: the definition the HIP kernels (csrc/sinkhorn.hip) are held to.

The reference `CoarseMatching(match_type='sinkhorn')` (src/matcher/utils/coarse_matching.py:121-143) imports
`log_optimal_transport` from a `superglue.py` it does not ship.  `log_optimal_transport` below is that one function, written
from the published algorithm (SuperGlue, Sarlin et al. 2020, section 3.2 and appendix: log-domain Sinkhorn with a dustbin row
and column that share one learned score):

    Z [L+1, S+1]: scores bordered by alpha;  norm = -log(L + S)
    log_mu = [norm] * L + [log(S) + norm];  log_nu = [norm] * S + [log(L) + norm]
    u = v = 0;  iters times:  u = log_mu - logsumexp_j(Z + v);  v = log_nu - logsumexp_i(Z + u)
    returns Z + u + v - norm

It is the stand-in scripts/gen_golden_sinkhorn.py hands to the reference module, and in fp64 the yardstick of the tests.  The
product path never imports this file.
"""
import torch

NEG_FILL = 1e9   # coarse_matching.py:6


def potentials(scores, alpha, iters):
    """(Z [b, L+1, S+1], u [b, L+1], v [b, S+1], norm, log_mu, log_nu) after `iters` iterations, in the dtype of `scores`."""
    b, m, n = scores.shape
    alpha = torch.as_tensor(alpha).to(scores).reshape(())
    z = scores.new_empty(b, m + 1, n + 1)
    z[:, :m, :n] = scores
    z[:, m, :] = alpha
    z[:, :, n] = alpha
    ms, ns = scores.new_tensor(float(m)), scores.new_tensor(float(n))
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])[None].expand(b, -1)
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])[None].expand(b, -1)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(int(iters)):
        u = log_mu - torch.logsumexp(z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(z + u.unsqueeze(2), dim=1)
    return z, u, v, norm, log_mu, log_nu


def log_optimal_transport(scores, alpha, iters):
    """[b, L+1, S+1] log assignment, dustbins included."""
    z, u, v, norm, _, _ = potentials(scores, alpha, iters)
    return z + u.unsqueeze(2) + v.unsqueeze(1) - norm


@torch.no_grad()
def assignment(feat0, feat1, bin_score, skh_iters=3, mask0=None, mask1=None):
    """exp(log assignment) [n, L+1, S+1] of coarse features [n, L, C] / [n, S, C]: similarity of feat / sqrt(C) without a
    temperature, the -1e9 fill where mask0[i] * mask1[j] == 0 (coarse_matching.py:123-132)."""
    c = feat0.shape[-1]
    sim = torch.einsum("nlc,nsc->nls", feat0 / c ** .5, feat1 / c ** .5)
    if mask0 is not None:
        sim.masked_fill_(~(mask0.flatten(1)[..., None] * mask1.flatten(1)[:, None]).bool(), -NEG_FILL)
    return log_optimal_transport(sim, bin_score, skh_iters).exp()


@torch.no_grad()
def conf_matrix(feat0, feat1, bin_score, skh_iters=3, skh_prefilter=True, mask0=None, mask1=None):
    """[n, L, S] confidence of the eval path: the assignment without its dustbins, rows and columns whose largest entry is
    their dustbin zeroed when `skh_prefilter` (coarse_matching.py:133-140; torch.max returns the first maximum)."""
    a = assignment(feat0, feat1, bin_score, skh_iters, mask0, mask1)
    L, S = a.shape[1] - 1, a.shape[2] - 1
    conf = a[:, :L, :S].clone()
    if skh_prefilter:
        drop0 = (a.max(dim=2)[1] == S)[:, :L]
        drop1 = (a.max(dim=1)[1] == L)[:, :S]
        conf[drop0[..., None].expand(-1, -1, S)] = 0
        conf[drop1[:, None].expand(-1, L, -1)] = 0
    return conf


def dustbin_margins(a):
    """Per row and per column of an assignment [n, L+1, S+1]: |dustbin - best real entry| / max of the two (the quantity the
    prefilter decides on; 1.0 where both are 0).  Returns (rows [n, L], columns [n, S])."""
    L, S = a.shape[1] - 1, a.shape[2] - 1

    def rel(bin_, best):
        top = torch.maximum(bin_, best)
        return torch.where(top > 0, (bin_ - best).abs() / top.clamp_min(1e-300), torch.ones_like(top))
    return rel(a[:, :L, S], a[:, :L, :S].max(dim=2)[0]), rel(a[:, L, :S], a[:, :L, :S].max(dim=1)[0])
