#!/usr/bin/env python3
"""Record what tests/test_model_io.py needs from the reference where the reference is absent.

Runs the reference (imported by path from ``$VBN_REFERENCE``; nothing of it is copied) and
writes ``tests/golden/recorded/model_io.pt``:

* ``log_prob[name][node]``: the reference model's log_prob (loaded from the fixture's own
  checkpoint) on the seeded inputs of ``test_reference_loads_our_checkpoint``;
* ``state_shapes[cfg][node]``: {state_dict key: shape} of every CPD after the reference loaded
  our random-init checkpoint (strict ``load_state_dict``), as in
  ``test_random_init_models_load_in_the_reference``.

    python tests/golden/make_golden_model_io.py
"""
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import test_model_io as T  # noqa: E402


def main():
    assert T.HAVE_REF, "set VBN_REFERENCE to the reference checkout"
    sys.path.insert(0, T.REF)
    os.environ.setdefault("CI", "1")
    import vbn
    out = {"log_prob": {}, "state_shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in T.REF_FIXTURES:
            fx = T.load_golden(name)
            model = T.model_from_checkpoint(fx["model"])
            p = os.path.join(tmp, "theirs.pt")
            torch.save(fx["model"], p)
            b = vbn.VBN.load(p, map_location="cpu")
            out["log_prob"][name] = {}
            for node, x, par in T.probe_inputs(model):
                with torch.no_grad():
                    out["log_prob"][name][node] = b.nodes[node].log_prob(x, par).clone()
        for cfg_name in T.REF_CONFIGS:
            model = T.small_random_init(cfg_name)
            p = os.path.join(tmp, "m.pt")
            T.VBN.from_model(model, device="cpu").save(p)
            r = vbn.VBN.load(p, map_location="cpu")
            out["state_shapes"][cfg_name] = {
                node: {k: list(v.shape) for k, v in r.nodes[node].state_dict().items() if isinstance(v, torch.Tensor)}
                for node in model.topo}
    os.makedirs(os.path.join(HERE, "recorded"), exist_ok=True)
    dst = os.path.join(HERE, "recorded", "model_io.pt")
    torch.save(out, dst)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
