// Drives PassPlan (gatb-core_amd/csrc/gkc_pass_plan.hpp) the way gkc_count_pass does, without a GPU: the optional probe batch, settle(), then the lanes
// carving in turn (lane 0, lane 1, ..., then each reports its batch finished). Reads "name value" pairs and "parts N v0 v1 ..." from stdin, prints one line per
// event; tests/test_pass_plan.py checks the properties.
//   g++ -std=c++17 -I gatb-core_amd/csrc -o pass_plan_driver tests/pass_plan_driver.cpp -lpthread
#include "gkc_pass_plan.hpp"
#include <inttypes.h>
#include <iostream>
#include <string>

int main()
{
    PassPlanInputs in;
    std::vector<uint64_t> part_keys;
    double d_true = 0.03;                    // solid records per key the simulated batches come out with
    std::string name;
    while (std::cin >> name) {
        if (name == "parts") { size_t n; std::cin >> n; part_keys.resize(n); for (auto& v : part_keys) std::cin >> v; }
        else if (name == "avail_bytes") std::cin >> in.avail_bytes;
        else if (name == "reserve_bytes") std::cin >> in.reserve_bytes;
        else if (name == "key_words") std::cin >> in.key_words;
        else if (name == "nb_passes") std::cin >> in.nb_passes;
        else if (name == "sink") std::cin >> in.sink;
        else if (name == "key_budget") std::cin >> in.key_budget;
        else if (name == "batch_cap") std::cin >> in.batch_cap;
        else if (name == "d_hint") std::cin >> in.d_hint;
        else if (name == "last_plan_budget") std::cin >> in.last_plan_budget;
        else if (name == "lanes") std::cin >> in.lanes;
        else if (name == "batch_keys") std::cin >> in.batch_keys;
        else if (name == "sink_first_div") std::cin >> in.sink_first_div;
        else if (name == "d_true") std::cin >> d_true;
        else { fprintf(stderr, "unknown input %s\n", name.c_str()); return 2; }
    }
    PassPlan plan(part_keys, in, [] { printf("trim\n"); }, [](uint32_t p) { printf("empty %u\n", p); });
    printf("start total_keys %" PRIu64 " lanes %d probe_pending %d probe_wanted %d probe_keys %zu\n", plan.total_keys, plan.lanes, (int)plan.probe_pending, (int)plan.probe_wanted(), plan.probe_keys);
    auto keys_of = [&](const std::vector<uint32_t>& b) { uint64_t k = 0; for (uint32_t p : b) k += part_keys[p]; return k; };
    auto show = [&](const char* what, int lane, const std::vector<uint32_t>& b) {
        bool consecutive = true; for (size_t i = 1; i < b.size(); i++) { for (uint32_t p = b[i - 1] + 1; p < b[i]; p++) consecutive = consecutive && part_keys[p] == 0; consecutive = consecutive && b[i] > b[i - 1]; }
        printf("%s lane %d first %u last %u n %zu keys %" PRIu64 " consecutive %d tight %d\n", what, lane, b.front(), b.back(), b.size(), keys_of(b), (int)consecutive, (int)plan.tight);
    };
    std::vector<uint32_t> batch;
    if (plan.probe_wanted() && plan.carve_probe(batch)) {
        show("probe", 0, batch);
        const uint64_t keys = keys_of(batch);
        plan.probe_finished(keys, (uint64_t)((double)keys * d_true));
    }
    plan.settle();
    printf("settled budget %zu lanes %d plan_lanes %d slots_hint %" PRIu64 " d_hint %.6f last_plan_budget %zu\n", plan.fixed_budget, plan.lanes, plan.plan_lanes, plan.slots_hint(), plan.d_hint, plan.last_plan_budget);
    const int lanes = plan.lanes;
    std::vector<std::vector<uint32_t>> cur(lanes);
    std::vector<bool> alive(lanes, true);
    for (int running = lanes; running > 0;) {
        for (int l = 0; l < lanes; l++) if (alive[l]) {
            if (plan.carve(cur[l], l)) show("batch", l, cur[l]);
            else { alive[l] = false; running--; printf("retired lane %d tight %d\n", l, (int)plan.tight); }
        }
        for (int l = 0; l < lanes; l++) if (alive[l]) { const uint64_t keys = keys_of(cur[l]); plan.finished(l, keys, (uint64_t)((double)keys * d_true)); }
    }
    printf("end rc %d\n", plan.rc());
    return 0;
}
