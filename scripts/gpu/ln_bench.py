import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from protopformer_amd import ops
M, D = 256 * 197, 384
dev = "cuda"
torch.manual_seed(0)
def timeit(fn, iters=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
x = torch.randn(M, D, device=dev); dy = (torch.randn(M, D, device=dev) * 0.1).bfloat16(); w = torch.randn(D, device=dev)
mean = x.mean(1); rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-6)
dres = torch.randn(M, D, device=dev); dx = torch.empty_like(dres); cast = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
dw = torch.zeros(D, device=dev); db = torch.zeros(D, device=dev); dnb = torch.zeros(D, device=dev)
rs = torch.ones(256, device=dev)
t_full = timeit(lambda: ops.layernorm_bwd(dy, x, w, mean, rstd, dw, db, dres_in=dres, dx_out=dx, cast_out=cast, rowscale=rs, rows_per_group=197, dbias_next=dnb))
t_nocol = timeit(lambda: ops.layernorm_bwd(dy, x, w, mean, rstd, None, None, dres_in=dres, dx_out=dx, cast_out=cast, rowscale=rs, rows_per_group=197))
y = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
t_fwd = timeit(lambda: ops.layernorm_fwd(x, w, w, 1e-6))
print(f"ln_bwd full {t_full:.1f} us | without column sums {t_nocol:.1f} us | ln_fwd {t_fwd:.1f} us   (bytes bwd: {(M*D*(2+4+4+4+2))/1e6:.0f} MB)")
# the two forms of ln_bwd2_kernel alone, alternating (test hook ppf_layernorm_test_bwd_path: 1 parent, 2 lean): python ln_bench.py [ROUNDS]
from protopformer_amd import _lib
full = lambda: ops.layernorm_bwd(dy, x, w, mean, rstd, dw, db, dres_in=dres, dx_out=dx, cast_out=cast, rowscale=rs, rows_per_group=197, dbias_next=dnb)
nocol = lambda: ops.layernorm_bwd(dy, x, w, mean, rstd, None, None, dres_in=dres, dx_out=dx, cast_out=cast, rowscale=rs, rows_per_group=197)
try:
    for i in range(int(sys.argv[1]) if len(sys.argv) > 1 else 5):
        t = {}
        for path in (1, 2):
            _lib.call("ppf_layernorm_test_bwd_path", path)
            t[path] = (timeit(full, 50), timeit(nocol, 50))
        print(f"round {i}: full (with the reduce launch) parent {t[1][0]:.1f} us lean {t[2][0]:.1f} us | without column sums parent {t[1][1]:.1f} us lean {t[2][1]:.1f} us")
finally:
    _lib.call("ppf_layernorm_test_bwd_path", 0)
