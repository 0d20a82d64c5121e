"""Generate the Ising trace fixtures from the REFERENCE scenario code (build container only).

    python tests/golden/make_ising_sweep_fixtures.py

As make_ising_fixtures.py records its own: the reference Ising scenario (examples/ising_model/Ising.py) and world
(multiagent/core.py) are imported from the reference checkout and run under the restated env glue (Env) and the
script's loop (main_MFQ_Ising.py:84-159), here with the two figures the script prints every step added: sum(reward)
(:158) and mse (:125-133, the terms added in act_group order against the script's reward_target table).
Output: tests/golden/ising_sweep_<case>.npz -- arrays only, the run's arguments among them as 0-d arrays.
"""
import os

import numpy as np

from make_ising_fixtures import Env, load_scenario

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    "n16_t08": dict(n_agents=16, temperature=0.8, act_rate=1.0),
    "n16_t002_act05": dict(n_agents=16, temperature=0.02, act_rate=0.5),
    "n100_t002": dict(n_agents=100, temperature=0.02, act_rate=1.0),
    "n100_t08_act05": dict(n_agents=100, temperature=0.8, act_rate=0.5),
}
COMMON = dict(steps=200, lr=0.1, decay_rate=0.8, decay_gap=7, seed=13)


def run(n_agents, temperature, steps, lr, act_rate, decay_rate, decay_gap, seed):
    np.random.seed(seed)
    sc = load_scenario()
    world = sc.make_world(num_agents=n_agents, agent_view=1)
    env = Env(sc, world)
    n_actions = 2
    reward_target = np.array([[2, -2], [1, -1], [0, 0], [-1, 1], [-2, 2]])      # main_MFQ_Ising.py:77-81
    obs = np.stack(env.reset())
    spins0 = np.array([a.state.spin for a in world.agents], dtype=np.int8)
    Q = np.zeros((n_agents, 5, n_actions))
    current_t = 0.3
    max_order, done_ = 0.0, 0
    orders, nups, rsums, mses = [], [], [], []
    for t in range(steps):
        action = np.zeros(n_agents, dtype=np.int32)
        if t % decay_gap == 0:
            current_t *= decay_rate
        if current_t < temperature:
            current_t = temperature
        for i in range(n_agents):
            s = np.count_nonzero(obs[i] == 1)
            vals = [np.exp(Q[i, s, k] / current_t) for k in range(n_actions)]
            denom = 0
            for v in vals:
                denom += v
            action[i] = np.random.choice(n_actions, 1, p=[v / denom for v in vals])[0]
        obs_, reward, done, order_param, ups, downs = env.step(np.expand_dims(action, axis=1))
        obs_ = np.stack(obs_)
        mse = 0
        act_group = np.random.choice(n_agents, int(act_rate * n_agents), replace=False)
        for i in act_group:
            s = np.count_nonzero(obs[i] == 1)
            Q[i, s, action[i]] = Q[i, s, action[i]] + lr * (reward[i][0] - Q[i, s, action[i]])
            mse += np.power((Q[i, s, action[i]] - reward_target[s, action[i]]), 2)
        mse /= n_agents
        obs = obs_
        orders.append(order_param)
        nups.append(ups)
        rsums.append(float(sum(reward)[0]))
        mses.append(float(mse))
        if order_param > max_order:
            max_order = order_param
        if abs(max_order - order_param) < 0.001:
            done_ += 1
        else:
            done_ = 0
        if done_ == 500 or t > steps:
            break
    return {"spins0": spins0, "order": np.array(orders), "n_up": np.array(nups, dtype=np.int32),
            "reward_sum": np.array(rsums), "mse": np.array(mses), "q_final": Q,
            "spins_final": np.array([a.state.spin for a in world.agents], dtype=np.int8),
            "stop": np.int32(len(orders))}


def main():
    for name, kw in CASES.items():
        args = dict(COMMON, **kw)
        out = run(**args)
        out.update({"arg_" + k: np.asarray(v) for k, v in args.items()})
        np.savez_compressed(os.path.join(HERE, "ising_sweep_%s.npz" % name), **out)
        print(name, int(out["stop"]), float(out["order"][-1]), float(out["mse"][-1]))


if __name__ == "__main__":
    main()
