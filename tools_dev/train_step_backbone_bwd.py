"""Backbone-backward window of the last training step in a rocpd trace: from the first bias_act_bwd kernel of the step (the first
ConvBNAct node to run backward) to the optimizer; kernel time grouped by kind."""
import re, sqlite3, sys
cur = sqlite3.connect(sys.argv[1]).cursor()
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table','view')")]
kt = "kernels" if "kernels" in tabs else [t for t in tabs if t.startswith("kernels")][0]
rows = list(cur.execute(f"select name, start, end from {kt} order by start"))
marks = [i for i, r in enumerate(rows) if "FusedOptimizerTensorListMetadata" in r[0] or ("multi_tensor_apply_kernel" in r[0] and "Adam" in r[0])]
groups = []
for i in marks:
    if groups and i - groups[-1][-1] < 40: groups[-1].append(i)
    else: groups.append([i])
lo, hi = groups[-2][-1] + 1, groups[-1][-1] + 1
step = rows[lo:hi]
busy = sum(e - s for _, s, e in step) / 1e6
first = next(i for i, r in enumerate(step) if "bias_act_bwd" in r[0])
opt = groups[-1][0] - lo
win = step[first:opt]
def kind(n):
    if "conv1x1_wgrad" in n: return "own conv1x1_wgrad (+reduce)"
    if "bias_act_bwd" in n: return "own bias_act_bwd"
    if "conv_bn_fold" in n: return "own conv_bn_fold"
    if re.search(r"conv1x1|mfma_pack", n): return "own conv1x1 forward kernel as dgrad (+pack)"
    if re.search(r"miopen|MIOpen|ck::|Cijk|igemm|gemm|naive_conv|wrw|bwd_data|SubTensor|transpose|batched_transpose|Conv|conv", n): return "MIOpen / CK / rocBLAS conv + layout"
    return "other (elementwise, clip, casts)"
agg = {}
for n, s, e in win:
    k = kind(n); a = agg.setdefault(k, [0, 0.0]); a[0] += 1; a[1] += (e - s) / 1e6
print(f"step: {len(step)} kernels, busy {busy:.2f} ms;  backward backbone + clip window: {len(win)} kernels, {sum(e - s for _, s, e in win) / 1e6:.2f} ms")
for k, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print(f"    {t:7.2f} ms {c:5d}  {k}")
names = {}
for n, s, e in win:
    a = names.setdefault(n[:100], [0, 0.0]); a[0] += 1; a[1] += (e - s) / 1e6
for n, (c, t) in sorted(names.items(), key=lambda kv: -kv[1][1])[:25]:
    print(f"      {t:7.3f} ms {c:5d}  {n}")
