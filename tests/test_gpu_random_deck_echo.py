"""Random deck sessions with the echo on the device (tests/random_decks.py session(echo=True); include/mixlab_gpu.h "ECHO"):
the sessions of tests/test_gpu_random_decks.py with set_echo calls between the runs and schedule_echo calls inside them on two decks in three -- several
echoing decks in one feed in shuffled order beside decks without one, on plain and key-locked decks, under loads, set_keylock calls and runs the deck sits
out, at every tick length of the suite.  Every materialised port, every deck record, mx_deck_debug_last_echo summed over the run's feeds and every deck's
echo_state, of the fused, unfused, one-tick and second-stream builds, against the models and the oracle bit for bit: the one-tick build takes the one-block
kernel where the others walk, so their equality is the header's "IT FOLLOWS" on random input.  tests/test_cpu_random_deck_echo.py shows what these seeds
cover and that each way the device could get such a session wrong changes something compared here."""
import pytest

import random_decks as rd
from mixlab_amd import abi
from random_taps import SETS
from test_gpu_random_graphs import ALL_SETS_RUNS, run_full_graph

pytestmark = pytest.mark.gpu

SEEDS = [("44k1", 200), ("44k1", 204), ("44k1", 210), ("44k1", 213), ("48k", 301), ("48k", 302), ("48k", 306), ("48k", 309), ("44k1_100", 400), ("16k_1000", 501),
         ("8k_8000", 601)]
TAP_SEEDS = [("44k1", 210), ("48k", 306), ("16k_1000", 501)]
BUILDS = ("fused", "unfused", "ticked", "overlap")


@pytest.mark.parametrize("shape_id,seed", SEEDS, ids=[f"{s}-{n}" for s, n in SEEDS])
def test_random_deck_echo_session_matches_the_models(shape_id, seed):
    run_full_graph(shape_id, seed, BUILDS, abi.FLAG_EQ_EXACT, decks=rd.session(echo=True))


@pytest.mark.parametrize("shape_id,seed", TAP_SEEDS, ids=[f"{s}-{n}" for s, n in TAP_SEEDS])
def test_random_deck_echo_session_every_tap_set(shape_id, seed):
    run_full_graph(shape_id, seed, BUILDS, abi.FLAG_EQ_EXACT, tap_sets=SETS, n_runs=ALL_SETS_RUNS, decks=rd.session(echo=True))
