"""The double backward of an MLP with softplus hidden layers, restated in torch in a given dtype (the formulas of csrc/mlp_softplus2.hip
k_mlp_bwd2_sp / include/nr3d_hip.h nr3d_mlp_softplus_backward_backward), and torch's own double backward of the same network.

Notation per sample: h_0 = x; hidden layers z_l = W_l h_{l-1} + b_l, h_l = softplus(z_l), s_l = sigmoid(beta z_l), e_l = 1 - s_l, with
s = 1 and e = 0 EXACTLY above the threshold (beta z > 20: torch's softplus double backward is 0 there); output layer z_L with the mask m_L
of an output ReLU.  u = dL/dy, v = dL/d(dL/dx):
    r_L = m_L u,  g_l = W_{l+1}^T r_{l+1},  r_l = s_l g_l                     (the first backward)
    t_0 = v,  t_l = s_l (W_l t_{l-1}),  dL/d(dL/dy) = m_L W_L t_NH            (the tangent of v)
    q_l = beta e_l g_l t_l,  p_NH = q_NH,  p_l = q_l + s_l W_{l+1}^T p_{l+1}  (the sigma'' chain, hidden layers)
    dW_l = sum r_l t_{l-1}^T + p_l h_{l-1}^T (output layer: the first term),  db_l = sum p_l (hidden),  dL/dx = W_1^T p_1
Both functions return (dL/d(dL/dy), dL/dx, [dW_l], [db_l | None]); db of the output layer is None (its bias does not reach dL/dx)."""
import torch

THRESHOLD = 20.0


def restated(ws, bs, x, u, v, beta, out_relu=False, dtype=torch.float64):
    ws = [w.detach().to(dtype) for w in ws]
    bs = [None if b is None else b.detach().to(dtype) for b in bs]
    x, u, v = (t.detach().to(dtype) for t in (x, u, v))
    nh = len(ws) - 1
    hs, ts, ss, es = [x], [v], [None], [None]
    for l in range(nh):
        z = torch.nn.functional.linear(hs[-1], ws[l], bs[l])
        sat = beta * z > THRESHOLD
        s = torch.where(sat, torch.ones_like(z), torch.sigmoid(beta * z))
        e = torch.where(sat, torch.zeros_like(z), torch.sigmoid(-beta * z))
        hs.append(torch.where(sat, z, torch.log1p(torch.exp(torch.where(sat, torch.zeros_like(z), beta * z))) / beta))
        ts.append(s * torch.nn.functional.linear(ts[-1], ws[l]))
        ss.append(s); es.append(e)
    zo = torch.nn.functional.linear(hs[-1], ws[nh], bs[nh])
    m = (zo > 0).to(dtype) if out_relu else torch.ones_like(zo)
    r = m * u
    dgy = m * torch.nn.functional.linear(ts[-1], ws[nh])
    dWs, dbs = [None] * (nh + 1), [None] * (nh + 1)
    dWs[nh] = r.t() @ ts[nh]
    g, pb = r @ ws[nh], None
    for l in range(nh, 0, -1):                                  # hidden layer l (1-based) = ws[l - 1]
        s, e = ss[l], es[l]
        r = s * g
        p = beta * e * g * ts[l]
        if pb is not None:
            p = p + s * pb
        dWs[l - 1] = r.t() @ ts[l - 1] + p.t() @ hs[l - 1]
        dbs[l - 1] = None if bs[l - 1] is None else p.sum(0)
        g, pb = r @ ws[l - 1], p @ ws[l - 1]
    return dgy, pb, dWs, dbs


def torch_double_backward(ws, bs, x, u, v, beta, out_relu=False, dtype=torch.float64):
    """autograd: dx = grad(y, x, u, create_graph), then the gradients of <dx, v>"""
    ws = [w.detach().to(dtype).requires_grad_(True) for w in ws]
    bs = [None if b is None else b.detach().to(dtype).requires_grad_(True) for b in bs]
    xi = x.detach().to(dtype).clone().requires_grad_(True)
    g = u.detach().to(dtype).clone().requires_grad_(True)
    h = xi
    for l, (W, b) in enumerate(zip(ws, bs)):
        h = torch.nn.functional.linear(h, W, b)
        if l + 1 < len(ws):
            h = torch.nn.functional.softplus(h, beta, THRESHOLD)
        elif out_relu:
            h = torch.relu(h)
    dx, = torch.autograd.grad(h, xi, g, create_graph=True)
    hidden_b = [b for b in bs[:-1] if b is not None]
    got = torch.autograd.grad((dx * v.detach().to(dtype)).sum(), [g, xi, *ws, *hidden_b], allow_unused=True)
    dgy, gx, dWs, rest = got[0], got[1], list(got[2:2 + len(ws)]), iter(got[2 + len(ws):])
    dbs = [None if b is None else next(rest) for b in bs[:-1]] + [None]
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    return zero(dgy, g), zero(gx, xi), [zero(w, W) for w, W in zip(dWs, ws)], [None if b is None else zero(d, b) for d, b in zip(dbs[:-1], bs[:-1])] + [None]


def make_params(dims, bias, seed=0, device="cpu"):
    """the 0.4 / 0.2 randn parameters of the fused MLP tests"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ws = [(torch.randn(dims[l + 1], dims[l], generator=g) * 0.4).to(device) for l in range(len(dims) - 1)]
    bs = [(torch.randn(dims[l + 1], generator=g) * 0.2).to(device) if bias else None for l in range(len(dims) - 1)]
    return ws, bs


def make_inputs(dims, n, seed=1, device="cpu", scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(n, dims[0], generator=g) * scale).to(device)
    u = torch.randn(n, dims[-1], generator=g).to(device)
    v = torch.randn(n, dims[0], generator=g).to(device)
    return x, u, v
