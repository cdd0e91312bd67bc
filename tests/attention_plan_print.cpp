// Prints the attention dispatch plan (unidisc_amd/csrc/attention_plan.h) of the cases it reads from stdin, one case per line:
//   D B H L sample_ids doc_ranges causal q_prescaled p_drop  q k v o do dq dk dv fwd_o (row strides)  fwd64 dq64 dkv64 dkv_ws dkv_pre tr_read  dev_cus plan_cus  name
// and answers, per line, the forward plan and the backward plan (p_drop goes through attn_drop_thr as in the entry points: a dropout call iff thr > 0).  Built and driven by tests/test_attention_plan.py with a host compiler: no HIP, no GPU.
#include "attention_plan.h"

#include <stdio.h>

static const char* const FWD[] = {"FWD_8WAVE", "FWD_GEN64"};
static const char* const DQ[] = {"DQ_8WAVE", "DQ_GEN64"};
static const char* const DKV[] = {"DKV_SINGLE", "DKV_HALVES_D256", "DKV_WS", "DKV_WS_PRE", "DKV_WS_SPLIT_SINGLE", "DKV_GEN64"};

static void print_grid(const char* name, bool chosen, const AttnGrid& g) {
  if (chosen) printf(" %s=%u/%u/%u/%u/%u", name, g.grid, g.nfull, g.hashalf, g.mg_nt, g.mg_H);
}

int main() {
  AttnProblem p{};
  AttnSwitches sw;
  int sid, ranges, causal, pre, dev_cus, plan_cus;
  float p_drop;
  long fwd_o;   // O's stride in the forward call (its `out`)
  char name[128];
  while (scanf("%d %d %d %d %d %d %d %d %f %ld %ld %ld %ld %ld %ld %ld %ld %ld %d %d %d %d %d %d %d %d %127s", &p.D, &p.B, &p.H, &p.L, &sid, &ranges, &causal, &pre, &p_drop, &p.q_stride,
               &p.k_stride, &p.v_stride, &p.o_stride, &p.do_stride, &p.out_stride, &p.out2_stride, &p.out3_stride, &fwd_o, &sw.fwd64, &sw.dq64, &sw.dkv64, &sw.dkv_ws, &sw.dkv_pre,
               &sw.tr_read, &dev_cus, &plan_cus, name) == 27) {
    p.sample_ids = sid; p.doc_ranges = ranges; p.causal = causal; p.q_prescaled = pre; p.dropout = attn_drop_thr(p_drop) > 0;
    AttnProblem pf = p;   // the forward call has no O input, dO, dQ, dK, dV
    pf.out_stride = fwd_o;
    pf.o_stride = pf.do_stride = pf.out2_stride = pf.out3_stride = 0;
    const AttnPlan f = attn_plan_fwd(pf, sw, dev_cus, plan_cus), b = attn_plan_bwd(p, sw, dev_cus, plan_cus);
    printf("%s fwd=%s dq=%s dkv=%s planes=%d", name, FWD[f.fwd], DQ[b.dq], DKV[b.dkv], (int)b.planes_needed);
    print_grid("fwd_grid", f.fwd == FWD_GEN64, f.fwd_grid);
    print_grid("dq_grid", b.dq == DQ_GEN64, b.dq_grid);
    print_grid("dkv_grid", b.dkv == DKV_GEN64, b.dkv_grid);
    printf("\n");
  }
  return 0;
}
