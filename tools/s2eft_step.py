"""GPU tool: the S2EFT config-5 train step (forward, weighted CE, backward, fused Adam) captured as one hipGraph and
replayed K times -- the bench leg alone, for A/B runs and rocprofv3 --kernel-trace.
--patches: the same step through `S2EFT(x1, x2)` (144 + 1 bands, patch 7: the token rows formed inside the gate kernel)
and through `ViT(tokens)` on the rows `neighbour_band_tokens` makes of the same patches, one graph each, timed in
alternating windows of K replays (ROUNDS of them each); prints every window and the two medians.
usage: python tools/s2eft_step.py [K] [side 0|1|2]
       python tools/s2eft_step.py --patches [K] [ROUNDS]"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402

import knobs  # noqa: F401,E402  (measurement switches: tools/knobs.py)
import vitcnn_amd.s2eft as S  # noqa: E402
from vitcnn_amd import CrossEntropyLoss  # noqa: E402
from vitcnn_amd.optim import AdamW  # noqa: E402


def captured_step(m, xs, t, crit, dev):
    """the model's train step on inputs xs, warmed up and captured: (graph, optimizer)"""
    opt = AdamW(m.parameters(), lr=5e-4, weight_decay=0.0)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            crit(m(*xs), t).backward()
            opt.step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crit(m(*xs), t).backward()
        opt.step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize(dev)
    return graph, opt


def window(graph, k, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(k):
        graph.replay()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / k * 1e3


def patches(args):
    import statistics
    k = int(args[0]) if args else 200
    rounds = int(args[1]) if len(args) > 1 else 5
    dev = torch.device("cuda", 0)
    kw = dict(image_size=7, near_band=3, num_patches=144, num_classes=16, dim=64, depth=5, heads=4, mlp_dim=8,
              dropout=0.0, emb_dropout=0.0, mode="CAF")
    torch.manual_seed(0)
    a = S.S2EFT(**kw)
    b = S.ViT(**kw)
    b.load_state_dict(a.state_dict())
    a, b = a.to(dev).train(), b.to(dev).train()
    w = torch.ones(16, device=dev)
    w[0] = 0.0
    crit = CrossEntropyLoss(weight=w)
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(64, 144, 7, 7, generator=g).to(dev)
    x2 = torch.rand(64, 1, 7, 7, generator=g).to(dev)
    t = torch.randint(1, 16, (64,), generator=g).to(dev)
    tok = S.neighbour_band_tokens(x1, x2, 3)
    with torch.no_grad():      # same function of the same inputs before anything is timed
        same = torch.equal(a.eval()(x1, x2), b.eval()(tok))
    a.train(), b.train()
    ga, _oa = captured_step(a, (x1, x2), t, crit, dev)
    gb, _ob = captured_step(b, (tok,), t, crit, dev)
    ta, tb = [], []
    for r in range(rounds):
        ta.append(window(ga, k, dev))
        tb.append(window(gb, k, dev))
        print(f"round {r}: S2EFT(x1, x2) {ta[-1]:.4f} ms/step, ViT(tokens) {tb[-1]:.4f} ms/step ({k} replays each)",
              flush=True)
    print(f"s2eft --patches B=64 config 5 (eval logits bit-identical: {same}): S2EFT(x1, x2) median "
          f"{statistics.median(ta):.4f} ms/step (min {min(ta):.4f}, max {max(ta):.4f}), ViT(tokens) median "
          f"{statistics.median(tb):.4f} ms/step (min {min(tb):.4f}, max {max(tb):.4f}) over {rounds} alternating "
          f"windows of {k} graph replays", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--patches":
        return patches(sys.argv[2:])
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    if len(sys.argv) > 2:
        S._SIDE_STREAM = int(sys.argv[2])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = S.ViT(image_size=7, near_band=3, num_patches=144, num_classes=16, dim=64, depth=5, heads=4, mlp_dim=8,
              dropout=0.0, emb_dropout=0.0, mode="CAF").to(dev).train()
    w = torch.ones(16, device=dev)
    w[0] = 0.0
    crit = CrossEntropyLoss(weight=w)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(64, 145, 147, generator=g).to(dev)
    t = torch.randint(1, 16, (64,), generator=g).to(dev)
    graph, _opt = captured_step(m, (x,), t, crit, dev)
    ms = window(graph, k, dev)
    print(f"s2eft side={int(S._SIDE_STREAM)}: {ms:.4f} ms/step over {k} graph replays", flush=True)


if __name__ == "__main__":
    main()
