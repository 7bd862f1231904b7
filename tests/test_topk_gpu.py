"""pod_level_topk through the C ABI against torch.sort: exact top-k of every level's key list, sorted descending, for the
single-workgroup path (<= 2048 candidates), the sliced path (16 workgroups + last-one-merges) and its corner sizes; the
level-concatenated copy (cat_keys / cat_level / n_total) the gather kernels read; tickets left zeroed, counts untouched
(the gather kernel consumes them).  Beside random and skewed scores: all-equal scores (keys that differ in the index word alone) and a
top band of exactly k - 1, k, k + 1 keys, for what the one pass loop behind every size class can get wrong."""
import pytest
import torch

from pod_compare_amd import hip

pytestmark = pytest.mark.gpu


def make_keys(C, seed, skew):
    g = torch.Generator().manual_seed(seed)
    if skew:      # scores piled up in a narrow band: many keys share their top bytes (what a radix select finds hardest)
        scores = 0.7 + 1e-4 * torch.rand(C, generator=g)
    else:
        scores = torch.rand(C, generator=g) * 0.95 + 0.05
    idx = torch.randperm(C, generator=g)
    return pack_keys(scores, idx)


def pack_keys(scores, idx):
    return (scores.view(torch.int32).to(torch.int64) << 32) | (0xFFFFFFFF - idx.to(torch.int64))


def make_tied_keys(C, seed):
    """Every score the same: the keys differ in their low word only, so a select that starts at the highest differing bit starts
    inside the index, and one on the byte grid passes five bytes that narrow nothing."""
    g = torch.Generator().manual_seed(seed)
    return pack_keys(torch.full((C,), 0.7), torch.randperm(C, generator=g))


def make_band_keys(C, seed, m):
    """Exactly m keys in a top band (scores in [0.9, 0.95)), the rest in [0.06, 0.07), in shuffled positions."""
    g = torch.Generator().manual_seed(seed)
    scores = 0.06 + 0.01 * torch.rand(C, generator=g)
    scores[:m] = 0.9 + 0.05 * torch.rand(m, generator=g)
    return pack_keys(scores, torch.arange(C))[torch.randperm(C, generator=g)]


@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("counts,topk", [([1, 0, 5], 1000), ([63, 64, 65], 1000), ([700, 1024, 1500], 1000), ([2048, 2049, 5000], 1000),
                                         ([20000, 2268, 594], 1000), ([145152, 36288, 9072, 2268, 594], 1000),
                                         # the register-cached select's size classes: one workgroup (<= 16 384), 16 cached slices (<= 262 144),
                                         # the loop version beyond; k > 1024 makes the slices hand over 2048 survivors (final selection: loop version)
                                         ([16384, 16385, 2050], 1000), ([300000, 40000], 1000), ([145152, 9072, 3000], 2048), ([36288, 16000], 100),
                                         ([5000, 20000], 1), ([2049, 40000], 1024), ([2049, 40000], 1025)])
def test_level_topk_equals_sorted_prefix(counts, topk, skew):
    check_level_topk(topk, [make_keys(c, 10 * l + c, skew) for l, c in enumerate(counts)])


# 2049 keys: one workgroup, keys in registers; 16385: 16 register slices and a register final selection; 262200: slices longer than
# 16 384 keys, streamed; k = 1025: every slice hands over 2048 survivors, the final selection streams over zero-padded lists
@pytest.mark.parametrize("counts,topk", [([2049, 16385], 1000), ([262200, 2049], 1000), ([2049, 16385], 1025)])
def test_level_topk_of_tied_scores(counts, topk):
    check_level_topk(topk, [make_tied_keys(c, 7 * l + c) for l, c in enumerate(counts)])


@pytest.mark.parametrize("dm", [-1, 0, 1])
@pytest.mark.parametrize("counts,topk", [([5000, 40000], 1000), ([40000], 1025)])
def test_level_topk_with_a_top_band_of_about_k_keys(counts, topk, dm):
    """`excl < rem && rem <= incl` at equality, and `remaining` carried into the bucket below."""
    check_level_topk(topk, [make_band_keys(c, 3 * l + c, topk + dm) for l, c in enumerate(counts)])


def check_level_topk(topk, key_lists):
    lib, P = hip.load(), hip.ptr
    counts = [len(kk) for kk in key_lists]
    L = len(counts)
    cfg = hip.PodConfig()
    cfg.n_levels, cfg.topk = L, topk
    lv = (hip.PodLevel * L)()
    base, bases = 0, []
    for l, c in enumerate(counts):
        lv[l].anchor_base = base
        bases.append(base)
        base += c + 3                      # odd gaps: level lists need not be 16-byte aligned
    keys = torch.zeros(base, dtype=torch.int64)
    refs = []
    for l, (c, kk) in enumerate(zip(counts, key_lists)):
        assert len(torch.unique(kk)) == c and bool((kk > 0).all())   # the contract: distinct, non-zero keys
        keys[bases[l]:bases[l] + c] = kk
        refs.append(torch.sort(kk, descending=True)[0][:topk])
    dk = keys.cuda()
    cnt = torch.zeros(2 * L, dtype=torch.int32, device="cuda")
    cnt[:L] = torch.tensor(counts, dtype=torch.int32)
    sel = torch.full((L * topk,), -1, dtype=torch.int64, device="cuda")
    sc = torch.full((L,), -1, dtype=torch.int32, device="cuda")
    cat = torch.full((L * topk,), -1, dtype=torch.int64, device="cuda")
    cat_lv = torch.full((L * topk,), -1, dtype=torch.int32, device="cuda")
    nt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    for rnd in range(2):                   # second round: the gather kernel has consumed the counts, every level comes out empty
        hip.check(lib.pod_level_topk(cfg, lv, P(dk), P(cnt), P(sel), P(sc), P(cat), P(cat_lv), P(nt), hip.current_stream()), "pod_level_topk")
        torch.cuda.synchronize()
        assert int(cnt[L:].abs().sum()) == 0                       # tickets
        if rnd == 0:
            assert cnt[:L].cpu().tolist() == counts                # only read here
            assert sc.cpu().tolist() == [min(topk, c) for c in counts]
            for l in range(L):
                assert torch.equal(sel[l * topk:l * topk + len(refs[l])].cpu(), refs[l]), l
            n = sum(min(topk, c) for c in counts)
            assert int(nt.item()) == n
            assert torch.equal(cat[:n].cpu(), torch.cat(refs))
            assert cat_lv[:n].cpu().tolist() == [l for l, r in enumerate(refs) for _ in range(len(r))]
            cnt[:L] = 0                                            # what pod_gather_candidates / pod_gather_decode do
        else:
            assert sc.cpu().tolist() == [0] * L and int(nt.item()) == 0
