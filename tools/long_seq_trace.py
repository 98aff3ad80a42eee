#!/usr/bin/env python3
"""Work for rocprofv3 --kernel-trace --stats on 512-token sequences (encoders with a 512 ceiling):
  1,024 sequences of 512 tokens per encode, f16x3 and f32 (the 9-16-key-tile attention bucket at full load), then
  one 512-token request: eager (kernel by kernel) and as a hipGraph replay (fastpath.SingleRequestPath).
Wall times per call are printed as well (host-synchronised, so they include launch gaps)."""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.encoder import DeviceEncoder
from instacart_next_order_recommendation_amd.fastpath import SingleRequestPath
from instacart_next_order_recommendation_amd.search import DeviceIndex

N_SEQS, LEN, REPS = 1024, 512, 3
shape = syn.BertShape()
w = syn.synthetic_bert_weights(shape, seed=0)
rng = np.random.default_rng(0)
ids = rng.integers(0, shape.vocab_size, N_SEQS * LEN).astype(np.int32)
cu = (np.arange(N_SEQS + 1) * LEN).astype(np.int32)
ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()


def timed(label, fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    print(f"{label}: {(time.perf_counter() - t0) * 1e3 / reps:.3f} ms per call", flush=True)


for mode in ("f16x3", "f32"):
    enc = DeviceEncoder(w, shape, gemm_mode=mode, max_seq_length=LEN)
    timed(f"[{mode}] {N_SEQS} x {LEN} tokens", lambda: enc.encode_packed(ids_d, cu_d, LEN), REPS)
    enc.close()

enc = DeviceEncoder(w, shape, max_seq_length=LEN)
one = ids[:LEN].tolist()
timed(f"[f16x3] one {LEN}-token request, eager encode", lambda: enc.encode_ids([one]), 20)
ix = DeviceIndex(syn.synthetic_embeddings(49688, 384, seed=1))
fast = SingleRequestPath(enc, ix)
timed(f"[f16x3] one {LEN}-token request, graph replay (encode + top-20 search)", lambda: fast.run(one, 20), 20)
