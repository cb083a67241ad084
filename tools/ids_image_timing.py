"""Dev tool: attention forward / backward timing of 2-D relative ids at the image's position (MMT_IDS_2D_IMAGE, origin 2)
against MMT_IDS_2D at the `--ids2d` config-3 shape (B=4, S=4096 = 2 + 63^2 + 125, 12 heads, bf16, radius 64, 8 global
tokens, R=49, dropout 0.1; lean kernels), the two modes alternated, several rounds of device-event windows."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'multimodal-long-transformer-2021_amd'))
import json
import torch, mmt_amd
torch.manual_seed(0)
B, S, N, R = 4, 4096, 12, 49
dt = torch.bfloat16
q, k, v = (torch.randn(B, S, N, 64, device='cuda', dtype=dt) for _ in range(3))
emb = (torch.randn(R, N, 64, device='cuda') * 0.02).to(dt); bias = (torch.randn(R, N, device='cuda') * 0.02).to(dt)
def t(fn, n=200):
  for _ in range(10): fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(n): fn()
  e1.record(); torch.cuda.synchronize()
  return e0.elapsed_time(e1) / n * 1e3
res = {}
for r in (1, 2):
  pats = {mode: mmt_amd.AttentionPattern(local_radius=64, global_start=3971, n_global=8, id_mode=mode, max_dist=12,
                                         patches_per_row=63, core_layers=r, grid_start=2) for mode in (2, 3)}
  state = {}
  for mode, pat in pats.items():
    kw = dict(pattern=pat, dropout_p=0.1, dropout_seed=5)
    out, lse = mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw)
    state[mode] = (kw, out, lse, torch.randn_like(out))
  for rnd in range(4):
    for mode in (2, 3):
      kw, out, lse, dout = state[mode]
      f = t(lambda: mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw))
      b = t(lambda: mmt_amd.relative_attention_backward(dout, q, k, v, emb, bias, out, lse, **kw))
      res.setdefault(f'r={r} id_mode={mode}', []).append((round(f, 1), round(b, 1)))
for name, rows in res.items():
  print(name, 'fwd us', [x[0] for x in rows], 'bwd us', [x[1] for x in rows])
print(json.dumps(res))
