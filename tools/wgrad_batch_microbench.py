"""Times nefii_mlp_wgrad_f16h_batch alone: four layers of 512 x 512, P points (default 116 700: config 3's batch is of that
order), both operands in halves - the blocked kernel mlp_wgrad16t_batch_kernel plus its zero fill.  NEFII_LIB_PATH selects the
library, so two builds can be run alternately.  Prints five timings of 20 calls each and a checksum of dW and db.

    python tools/wgrad_batch_microbench.py [P]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefii_amd import _lib
lib = _lib.lib()
P, L, W = int(sys.argv[1]) if len(sys.argv) > 1 else 116700, 4, 512
dev = 'cuda:0'
g = torch.Generator(device=dev).manual_seed(1)
dz = (torch.randn(L, P, W, device=dev, generator=g) * 100).half()
x = (torch.randn(L, P, W, device=dev, generator=g).abs() * 16).half()
dW = torch.zeros(L, W, W, device=dev)
db = torch.zeros(L, W, device=dev)
S = torch.full((1,), 1024.0, device=dev)
items = (_lib.WgradItem * L)(*[_lib.WgradItem(dz[l].data_ptr(), x[l].data_ptr(), dW[l].data_ptr(), db[l].data_ptr(), W, W, 1, W, W, 1.0)
                               for l in range(L)])
st = torch.cuda.current_stream().cuda_stream
def run():
    rc = lib.nefii_mlp_wgrad_f16h_batch(items, L, P, S.data_ptr(), st)
    assert rc == 0, rc
for _ in range(5):
    run()
torch.cuda.synchronize()
ts = []
for rep in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        run()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / 20)
print('%s P=%d: ms per call (zero fill + 4 layers) %s  checksum %.6e %.6e' % (
    os.environ.get('NEFII_LIB_PATH', 'tree'), P, ' '.join('%.4f' % t for t in ts), dW.double().abs().sum().item(), db.double().abs().sum().item()))
