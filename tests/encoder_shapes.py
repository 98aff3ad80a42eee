"""Encoder shapes besides all-MiniLM-L6-v2 that icrec_encoder_create accepts (BertShape fields over vocab 2,048):
tests/test_encoder_shapes_gpu.py runs the HIP encoder at them, tests/test_oracle.py pins the oracle at them."""

SHAPES = {
    "layers1": dict(layers=1),
    "layers3": dict(layers=3),
    "layers12": dict(layers=12),
    "inter384": dict(layers=2, intermediate=384),
    "inter768": dict(layers=2, intermediate=768),
    "inter1152": dict(layers=2, intermediate=1152),
    "inter3072": dict(layers=2, intermediate=3072),
    "normalize3": dict(layers=2, n_normalize=3),
    "normalize4": dict(layers=2, n_normalize=4),
    "ln_eps1e-5": dict(layers=2, ln_eps=1e-5),
    "type_vocab1": dict(layers=2, type_vocab=1),
    "max_position64": dict(layers=2, max_position=64),
}
