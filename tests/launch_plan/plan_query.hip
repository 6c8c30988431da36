// plan_query.hip -- asks plan_objective (csrc/objective_plan.h) about ONE launch, on the CPU: no HIP call, no GPU.
// tests/test_gpu_pair_swarm_modes.py compiles it once and asks it, with the device's compute-unit count, which form
// and which mode of a swarm generation every one of its cases must reach; what the library then reports of the launch
// (nmrfit_last_launch, nmrfit_pso_last_launches) is held to the answer.
//   plan_query <compute_units> <S> <N> <P> <pair_waves: -1 | 0 | 1> <target_waves> <variant> <mode>
//   mode: objective | fused | fused+pbest | fused+pbest+tail | fused+pbest+tail+pending
// prints one line: code= unit= nseg= wpb= pair= waves= blocks= pbest= tail= rows= flush= lds=
#include "objective_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace nmrfit;

int main(int argc, char **argv)
{
    if (argc != 9) {
        fprintf(stderr, "usage: plan_query <compute_units> <S> <N> <P> <pair_waves> <target_waves> <variant> <mode>\n");
        return 2;
    }
    ObjectivePlanInput in{};
    in.compute_units = atoi(argv[1]);
    in.S = atoll(argv[2]);
    in.N = atoll(argv[3]);
    in.P = (int32_t)atoi(argv[4]);
    in.pair_waves = atoi(argv[5]);
    in.target_waves = atoll(argv[6]);
    in.variant = atoi(argv[7]);
    const char *mode = argv[8];
    if (strcmp(mode, "objective") != 0) {   // a swarm generation: what evaluate_and_select (csrc/pso.hip) passes
        if (strncmp(mode, "fused", 5) != 0) {
            fprintf(stderr, "plan_query: unknown mode '%s'\n", mode);
            return 2;
        }
        in.defer = in.fused = in.fused_rows = true;
        in.pbest = strstr(mode, "+pbest") != nullptr;
        in.tail = strstr(mode, "+tail") != nullptr;
        in.pending = strstr(mode, "+pending") != nullptr;
    }
    const ObjectivePlan p = plan_objective(in);
    static const char *const kUnits[] = {"none", "default", "farfield", "farfield32", "norec", "rows_im", "pair", "ab"};
    printf("code=%d unit=%s nseg=%d wpb=%d pair=%d waves=%lld blocks=%lld pbest=%d tail=%d rows=%d flush=%d lds=%lld\n", p.code,
           kUnits[(int)p.unit + 1], p.nseg, p.wpb, (int)p.pair, (long long)p.waves, (long long)p.blocks, (int)p.pbest, (int)p.tail, p.rows,
           (int)p.need_flush, (long long)p.lds);
    return 0;
}
