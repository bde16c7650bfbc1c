"""The named inputs of the region-map suites, pinned (no GPU).

PINNED holds the sha256 of every named input the suites build -- over the dtype
string, the shape and the bytes, and for a (map, R) pair over R as well -- taken
from the builders as they stood inside the GPU test modules, before they moved
to region_inputs.py.  Each test rebuilds its inputs through region_inputs.py
(the two 1100 x 1000 maps through test_regions_atsize_inputs.py) and compares,
so an edit to a builder that changes what a GPU test is fed shows here first.
A key is the builder's kind and its arguments, joined by "|"."""
import hashlib

import numpy as np
import pytest

import region_inputs as ri
import test_regions_atsize_inputs as atsize

PINNED = {
    "regions|noise3|1|1": "108b602ff2f3b759ca68d3bcd29259328cde167601280519907fdf3edb0e8438",
    "regions|noise3|7|1": "ab79619c3391243a71856c88e0f805e8b34324341691765e2858ec9256ef51f9",
    "regions|noise3|1|7": "f8e59d721a20da2504a5503e5bcb8d6370512b8cf084ad603865e83e76553d4d",
    "regions|noise3|64|64": "fbacdd696f5bdaf731c4661066f4ebd1c4b5fd9394b51648aceaecb66f7dd237",
    "regions|noise3|65|64": "0b83faa333fa15efc901b4447872405e97815705f281a73e9d5aef5fc07bac22",
    "regions|noise3|64|65": "15d20d3044340435517821332207433ba6692aaaf06afdf77fc620f98cd35bbf",
    "regions|noise3|65|65": "14e0254b29f5c7d199b90dcdec33184dab1b39c7d263ac61532d885ec6d979f1",
    "regions|noise3|191|191": "06b1ea2a624779170a9e1e7e504be9467389f38c815ab7cc676e5a52ac516223",
    "regions|noise3|66|5": "bd9f8375ef0f48b72b31031c4da21366310fa50d1121977df930984ce14e38ca",
    "regions|noise3|67|5": "a890c342a32c4f2357ac7fe253262a9dec3299b466e0c7347ef92c7fe50bc474",
    "regions|noise3|130|70": "f44b803eb28c0c1a29d7472f475444ccde4b059dbd326433248501da595f77d6",
    "regions|constant|200|150": "c7725dda58efdcfc05fe1c8a02c01be7caaad0301c68673f1a9fdf3aa84f0f4f",
    "regions|checker|200|150": "cb54ab385b2beb60ba9b0c5ead303c3d5da21a0efe9979af7b53e564c4c25912",
    "regions|hstripes|200|150": "70f8ccca2f707ae1d6129060f5ddc533effe1a592e57a86e6d6e762969d260da",
    "regions|vstripes|200|150": "2f9683c596ea02920782af60fbd54226b343566c014a7a272c8db329fc85ada8",
    "regions|spiral|200|150": "c6fe9f16934b9c2d6fe77d20edbaf5580f9def6e424298c4bdc6b9a97a855cdb",
    "regions|comb|200|150": "4626983027cbda93d4cdf0e9810eea5e8d4480e552cfaf29a26a9977a05b87d5",
    "regions|rings|200|150": "3e42812f420f4abe4aac795bf0a296de349f3a381d49aee3c51e6a49b9334dc9",
    "regions|diagonals|200|150": "6bd195d88c88920f56270fd1c6431df687310ae50ddc4b020059b6c36b518671",
    "regions|noise2|200|150": "35a32575edd1cdf98d88cc0462638fa22fd0ff4ee9c52c33c58f2530e084dca6",
    "regions|noise3|200|150": "2434f360527129bba365100a0af8ed4b96c68255e516a79d46726d6b3be6d8e4",
    "regions|noise200|200|150": "69098c0d85b3b10cd2adb1e0eb329f22b92b00f0f3f1cb69cd079661c0ccce1a",
    "regions|noise3|67|66": "a34fae3700079c4fded4e68bf00ad1d29026581a17a8d76ba5fc0e3ad5552b5f",
    "widen|noise3|200|150|1": "6fe02d2e06e9755943d835e90bd4d535bdb743e6300931c385fc0c18bf81227c",
    "widen|noise3|200|150|2": "8fed1eb6d8844ebe6288cad772b057ec1be7e8e6b667d86ac52accc13491d52e",
    "widen|noise3|200|150|4": "88e2276ef88c8939c008716ea249a8265f46696fa956530f10d4c9ac5a8f5599",
    "widen|noise200|200|150|1": "435d15a9b289c0d29c6e466784edf5163521804aba76eee5ba780ba90c2fb868",
    "widen|noise200|200|150|2": "b724e8de891036caeeecc8dee51a57b793f158b10e5f02715d49637c60be5240",
    "widen|noise200|200|150|4": "cf0c023d6b34dd89cfee06c9f15009ac231b85e22be6a5ac2ad6c9232b58a9b9",
    "widen|noise3|67|66|1": "f8c402ae0ff872f8fbbadaab4a681b4366f4b795994a6c9c137967f74e17dce0",
    "widen|noise3|67|66|2": "dfa68444e8df53daa3c1b0e3ac8d611b36a482048e2894a1dfd3f7983c3ec092",
    "widen|noise3|67|66|4": "b2f00e8906f1456fe8c1916d74f1fbf495441c36fa3d199f4d51861d6778a2b6",
    "noise|200|150|3|0|int64": "2434f360527129bba365100a0af8ed4b96c68255e516a79d46726d6b3be6d8e4",
    "noise|67|31|5|9|int64": "7f2348918c54c875f1d848ccb304b60ce584d56f6ca5bf09951ec7d1e4096372",
    "adjacency|arange|1|1": "72b0dfbf78b2868f33c0dfbfdabc76dc99a7b0c2b16c9a4faa977d048c4d870f",
    "adjacency|arange|1|9": "f0059f7755396ec6ebd29bbe7dc0a04721a8b709827e22f69afc51b7aed943c8",
    "adjacency|arange|9|1": "e5c9e39c7e9e9362c856114583b5e87eeb5a37d695c0c8ad3af86766c3844856",
    "adjacency|arange|2|2": "e3c9d25bfeddcb23d7b809b7b89d54ecff045e8536aeba7f7cd96e432b192185",
    "adjacency|arange|5|3": "da0063b7511d62e9a1ec49055aef3febc053bbb7043dc3d3ee3caa60664a7fdd",
    "adjacency|arange|63|3": "47c2653b521e528fb5ae75e454ac2c1951a45e2112125843a960cd3116c481f6",
    "adjacency|arange|64|3": "0285377c19b1c9f0592d81ade04128b90371aba5cd6fc41a7a425c7d35cfdff9",
    "adjacency|arange|65|3": "8b06eae415ecb31cf387164dc25499b32514e00d5c8f850f7943094a1b8ffaaf",
    "adjacency|arange|67|31": "bcf6a46e3410244182c9347ad9a836e87eed58e552d3982671c32de87da069f8",
    "adjacency|arange|1024|2": "aef1d7489419237ac375ef65869f7e873eebcf96c513e8b27aa71c416aaad603",
    "adjacency|arange|1025|2": "fe612fd08f1ffc29a9ebbd50cce1aa82ee311ce214573947034e34de4726f282",
    "adjacency|arange|32|33": "78dc0099f120d1cf674e98765f0057b4859ce16fa62ecc914fa7007b75b81abf",
    "adjacency|noise3|1|1": "81a51082e918a42dcce4afc8d160c1a9ef921c81f2acdf7e50eff8fdd695689a",
    "adjacency|noise3|1|9": "8b9f12f9d9d3a8b72d59787b9107b144593c19e10d805bf6756da6eb42efd05a",
    "adjacency|noise3|9|1": "24ca339574506bb7d1d5eaaf5b1513d5a0709d7946c977886a1b0e22bace0770",
    "adjacency|noise3|2|2": "570a2840b5e96985a51759998f56352f6dd1addaac70e1aeea89021f7340cf15",
    "adjacency|noise3|5|3": "ffa7211837b32166473acfbbbf11f7fd655ad9aa7834a51e1bf51a142f2751b0",
    "adjacency|noise3|63|3": "a20ac8918ac935736a7c04a395dd347693ef758fb5aa7989e71d187bb0c258ed",
    "adjacency|noise3|64|3": "268ef2a12c3942efbf329892d7afb20c93c74d0b300c5a7e7fea759dce264f84",
    "adjacency|noise3|65|3": "0b496e222b6541600340e3608e13849f2c1022602b57896663cd025c1ca5b2cc",
    "adjacency|noise3|67|31": "b690d692c09f10babd94b50864fd7927d3c197276ce20cd74e59a0a18c9c4ad7",
    "adjacency|noise3|1024|2": "dad6c9c868e5b6d1561527a91d6a65bfefe1fdec2721224c3cb31ab84b489d40",
    "adjacency|noise3|1025|2": "3616adeeb1863cc920f2c95fc07ba75c34c02ec7c2d6ae0ace8c297c843aa685",
    "adjacency|noise3|32|33": "f2d63474c8e52b4e2c1cdf4e2abe6190be5f1709626a6864ab2394f2a9950bbc",
    "adjacency|halves|256|40": "362acc7dc46894d482f56cb978b834ac84d0036eec75de8d9a6c57d1799cee32",
    "adjacency|quadrants|256|40": "e1564f597a201f54c1ce443603db94d52fb5f18002724d212386dc233f7e8b8b",
    "adjacency|vstripes|200|7": "e7ec1791d21d70be8fa8cb94584b2a9d74ba1599b54ae76ca5bdcb901abbbd4d",
    "adjacency|k4|66|34": "7b763ae6fdfe6eed16a7a462bfc1a3b7dfcb1da033ebb6bf1ce41f3634194071",
    "adjacency|checker|67|31": "51b4b92bae33087e193a5d0b839330d3ce30ebbb590a67f5fd33aee0dc699efc",
    "adjacency|constant|67|31": "1eddfadade9810f0b0427a8381c49e152b1e7f4d6ac55434f64af23be9c37fd4",
    "adjacency|noise7|130|70": "58c1368402609dc75130a945c618da6aed65e2169b1016888bbc6bb883471e86",
    "adjacency|noise50000|130|70": "3ece8ac6b4b0a9dd5d1b219a4efecb3829bbb9b040183336b7ded3eea45925e5",
    "adjacency|reversed|67|31": "d18d2c6b0a916131ecdf0dbfc75033554f8c424c2366f34b8170d2656ddc9333",
    "adjacency|permutation|67|31": "8af139429dc2bd12b0fd598e5b1c88240dfe7e4c799d8cc00182bb696e44ce6f",
    "adjacency|huge_ids|67|31": "c14593444a56e00570008617ac20db069e5c457b584c257e88b4d52f017d8003",
    "adjacency|noise7|67|31": "5ebef2ed932b70c3adf4ad3d199e381256723dc259cbbae5e2bd85b566ebc935",
    "noise|130|70|7|0|uint32": "58c1368402609dc75130a945c618da6aed65e2169b1016888bbc6bb883471e86",
    "noise|67|31|5|9|uint32": "ff84e458faeab1aef29a7e64e7bfea7427d3ecd1cdd3c87a94e496c5bb9aa8a2",
    "merge|noise64x48|labels": "3f4ea14c733d704b289c136c271f6cdb0706f0bf461a7cebb48c67b5f79a67ac",
    "merge|noise64x48|pixels": "e24af7c812b4c86ad67e5af38588f759454b483d1cff369f20d28e879962edd4",
    "merge|noise64x48|regions": "f6936032ff72a792be9a4cbaf258fba63f681c41661fd83d71bc357ae0cabf8f",
    "merge|noise64x48|edges": "93b0cd09153e94a057d4931a2f33b820aaf09c1fda5f7b6a294c1933eabafe23",
    "merge|noise96x80|labels": "ac34f10dab88c986e815e440863d51c314a21903dbb349f9db425ad78132dc98",
    "merge|noise96x80|pixels": "a1c158b4d834e84f6a8223a26098c381934f61951da01c15773b5e90b686123c",
    "merge|noise96x80|regions": "f5d2636e569e7aa7c106f2bf1cc5732158092fc3b68f0b80d62b12c9632f45ea",
    "merge|noise96x80|edges": "aa90ada35d9c4b67f60c8eb1e1c5397bd0622a3fcdbcc9136636d88c9b15a658",
    "merge|noise97x41|labels": "f55404331fd7ef20fe823be4547a2d24e7ca369a579c390768b851982e73807d",
    "merge|noise97x41|pixels": "152b0c175afb9a1a326e25462b88315c4511611f914a7cc98b680381bec90562",
    "merge|noise97x41|regions": "9d581f0bb5cbfd2b93e9a7b6a6d98689f06f61f831d23ab161fd4043103d01df",
    "merge|noise97x41|edges": "aa242b8cd5fc6b789d86500374e063c3b3fb0cd022e9693c7290acf71928c43d",
    "merge|chain|labels": "df6c59219820c9ff9181b968bba4b705ce02b6c3e69ba17bd4f858b74e0ac62d",
    "merge|chain|pixels": "a052f1027cc9aac0f7794e472da30713be51c6a571683367a486882416551e2f",
    "merge|chain|regions": "f731b60768176193d1382643dd425f36f3991e3c0d63d96130138cd76c264efc",
    "merge|chain|edges": "4de89dec04845ba93af1af120a17d5051928d71d16aa2aa717b78c60d388a7df",
    "merge|islands|labels": "7c608e9edb6109e4027d2b512e97ba2cd656010502ebb526fde17afe14599751",
    "merge|islands|pixels": "ebcf79ba95b8aa44308c0e56dc760a41e38d7617500ce24d0c135ef01e60ddc6",
    "merge|islands|regions": "20af7bad03e9e71d16fd1e1493512cbf04198ffd871a8ff8f896254032265718",
    "merge|islands|edges": "241941464df1098a5eea8016effdc34a2bacdbb6c59fa04f3dd7d00a2d192ede",
    "merge|stripes|labels": "2f2f4b70aa75f4ca350fa7df78ab936d99adb5c52d2c16bcc20c27d4ca5a2fa8",
    "merge|stripes|pixels": "341e01445fb4a4a395d596e76d4c810053a1b2a8ab5ce21049e6bc27b5bb457a",
    "merge|stripes|regions": "144486056e06ff97460f38c444db60867b59ff0728fea5ec8f55750f1c88c6e7",
    "merge|stripes|edges": "19329a46dc07f1c35830826560d42e901e0a777c57eb528be572b16def318d92",
    "merge|one|labels": "ba864443d69a913cfafcf22edddc0d15ef232f703d3e8914fa8f7ff66eb178d3",
    "merge|one|pixels": "c0e50a9521b682c75a0f04b0845377f71589469dab0ef998c9ece16baade576f",
    "merge|one|regions": "faed034815221ff04d7538cb7ec59934322eef29da24cb02329015a07e9d5ad8",
    "merge|one|edges": "eb33bce6f335f329078e8c494ad7d3475f4b15ee17d20bca40e85e22ca1dabec",
    "noise|64|48|4|1|uint32": "648b62440727959ce31ca070bbdbd7442aaf5b36c136867800e5d0af58097143",
    "noise|97|41|3|1|uint32": "bb8473a1acfb736815a57b12d8eef58245f8cd5444e1ec5b8edd362806d122c3",
    "noise|24|16|3|1|uint32": "2ceb57c573562c3d19c6820878dec96cc6cb0f188f1535d165d6ba7bd3cdf9da",
    "frame|1|1": "9a0bad78c36a7f3c9563a1c0076d08d18ba6c950640ce8b9b17c0ec6effd31ec",
    "frame|1|7": "da5d389e27a8bfa98e3cc58ad99d0ffcec2f95ac20b3103ab21a6a3bc7a0a0dc",
    "frame|1|2048": "fcd0c2c05ff345c908d665522df61de58e3709f27312be7757b0c9c4c0a788d8",
    "frame|3|5": "e384576b8502ce86024c1b7ce76bc7cdf63d6fe90d4736fcb7a5c106bf16a0d1",
    "frame|4|64": "8dd8194d54173762589e90700b26746ed3afc3c298ebe82083349c56f53c6f93",
    "frame|4|200": "d27659c424f09bf5e00b78988d986701fc70e337aae7c086b74d357a7a30ae46",
    "frame|7|5": "c7aa73b229bad474f3a19fb35f6667763f7b64c41c1e9e408a94af2058f67ef0",
    "frame|16|12": "a99a1d6b23d9deedfb9730c47ef270e0b09ffaaa32e40ee53f1f6c17ffb6d184",
    "frame|24|16": "ad922a55ec609a99414a3f573e66fa8dcea595de6dbeb4908d639ff877d9d8aa",
    "frame|40|40": "edfe92e425e677f1210737fa9ff7cdda23d7f2f805f2b55155dc8c37fe042610",
    "frame|45|37": "f252e5598f4abc4d24156bd4782551519bad76926a40bbebde5ac46178865ccf",
    "frame|63|3": "3cc3a152b131324a88b2950216c9ca34ea7d5d833ecfc1b061c4f98144beea1d",
    "frame|64|48": "41a373cb5de3682664f60b54431481810080c13a297ea14376df10de64f68c02",
    "frame|64|64": "231ec21a3d4f61ce57bc3a199e360bda979b8932892fdd6afe4ad1ba14ab2b53",
    "frame|67|31": "4e90f5cf82d0a99aec4c70c09727c6bfa2486cb9e22e044a6d02006507700c07",
    "frame|70|30": "e9b5ac5969e7d2a0a350e3b26c624730fa93d91997c5df9cbe9fed0b1cd8d4ac",
    "frame|96|80": "7500cbe6495c1018365dd6257c014357be8a712ebd570d5e7f7b10d80bfade0e",
    "frame|97|41": "791b8a226f458b36047811a91e5fd43bfbc453d0baa05c530c9939d6934bd782",
    "frame|129|3": "b7ecb3909e63e2f89f1909cb88d1d034a3f545c81d389cca89595fee595d22c1",
    "frame|130|70": "24d14e8430f1921f9852fb6b822d1fcf1bce1708696879a55a7f8dc344c3e5da",
    "frame|150|21": "761bd3aa0cd7d67e9dcf3c4323f41aad8baecc458a7e19ad6aefd6fc918b155c",
    "frame|200|5": "437d12b5bc696efe5c1038ccdf592f3c535e2cd5760cabfa4ffcafc8581660f3",
    "frame|200|150": "4ce5fb92bf61104ecb0473e14d3940e2da9d3746700cce9162f7b7271ca3a610",
    "frame|512|300": "34c54d30b1673ecbfa2339d048b73a95571ec8f3acfdf128fee88c7728314e19",
    "frame|1100|1000": "50d327fdb22c578223e184a2069a0be24b5c466b33c661e4d44e23967569c390",
    "frame|2048|1": "fcd0c2c05ff345c908d665522df61de58e3709f27312be7757b0c9c4c0a788d8",
    "pixels|noise64x48": "54f57bfb695831e0c7d35b17c35dbe04fa6ad03eb7bae324b49c21bc12326ef1",
    "pixels|noise96x80": "3d5b110fc2f8336b5d0e41f07ff3fa42e831baca6be77458cc83f05fef37e4fb",
    "pixels|noise97x41": "893274959e4fdde6d5edeb79f7c057e8ff567cff94c71e4e9935eb9ffac1e6df",
    "pixels|noise512x300": "dd2e904bde6ac561d67fb090cde6d8e73ca92f69109140fdc41852aea72bd90f",
    "pixels|noise64x48-permuted": "fe5920b57954f31fe48f9af0fc7ae6627a0e2e4416f1107e1fffb7dc64a58090",
    "pixels|noise96x80-permuted": "bacbdad6e767cb3f3df8b51aad0406d803ba417f931541a7c0a92d05b3574808",
    "pixels|noise97x41-permuted": "6cf54e013abaa6f613bcea05aeb977b7573bfd17903ced18f3654840fcb124f1",
    "pixels|rows1x7": "7bd18d5f3cd36c5d5fbf7820916408e6adefe4c11ca09255fbb85e3056e070a4",
    "pixels|rows3x5": "b60b1175c0d5d39bd261e0e25a3b054b640c841881d8ca46b198715edb050550",
    "pixels|rows63": "e3669a379c5013fb5dc530723c60fd7f56317c27aef949163db131f7939fbcac",
    "pixels|rows64": "07e626e97b498d244534984db4fe0a7e62c8ac8945428fc9df791350ef153d93",
    "pixels|rows65": "2959f131b07ef4040d4cdceb091a76bc176767a5ebd3cac21ecb31766e4d59ac",
    "pixels|rows129": "eb545bc434a36ad19591e4f8e0401bea5e3c48a51c5865a3859bd50732af6317",
    "pixels|stripes": "1d097e3683e65e066899176bfd844dfaba546deb17a2cf74ee5dc4a075b01163",
    "pixels|comb": "e621fa2de405e07af6c04469916ab3baf9e6da527a0a36a38f4dcca53a4267c5",
    "pixels|rings": "66ca107645ec98915fbda45c91b22bcfe4710f91587d1946d4fd47643761c346",
    "pixels|one": "41acc7d43dbeae95a3bc3c472e9adac1e1cd8d3a82a0231fc9042485c868d1bc",
    "pixels|each": "82a1de6422bc0edf3a116e89bf129a3ce401f7d11e811d8c2ab56be40860ab24",
    "pixels|line": "20d5a77e0c32a3b99054a44e29154a96cce142b2b73dd7cff599cc3f4b8d26bd",
    "pixels|column": "bd3fdd8675bbf5a73b581ffa908e338d3822f0d4374a20410753b6145c3fed09",
    "pixels|big": "c3f87dcc054a7be1543ca888f07472a3fc46557739dd8b12407dd999b7618220",
    "gaps|3|0|0": "3341d7e77e965bad7d692f952cc07f9762b26f21048ef389429b802e9c737df4",
    "gaps|0|2|0": "88a8144663106285ea7bb89c9f9bc4899198a5332d58658c18b69a480dfaf64f",
    "gaps|0|0|5": "aae3d387220b370bbef96b5178547d63260a0dd9639200aeb4e6352543d4fef8",
    "gaps|2|1|1030": "dd1ca244e575e703cddc6181a382325c725ae19db8dab0c072e9f0f1c6d4cef4",
    "gaps|2|1|7": "2bd1f5c5c1673cb0ac75d2d76171c7de823bcf1aea6ff98899b4408a90d54744",
    "permuted|noise97x41|7": "56c464ef058af105bda3604884c835e0388f6626838d1d8fb0725545f14c8cec",
    "relabel|rings": "bfe953a4b1521249dd1d711c83d3f2ba4d088a4628cdc58c72a2ab0629645ca3",
    "wmap|rows65": "2959f131b07ef4040d4cdceb091a76bc176767a5ebd3cac21ecb31766e4d59ac",
    "wmap|comb": "e621fa2de405e07af6c04469916ab3baf9e6da527a0a36a38f4dcca53a4267c5",
    "wmap|noise97x41": "893274959e4fdde6d5edeb79f7c057e8ff567cff94c71e4e9935eb9ffac1e6df",
    "wmap|rows3x5": "b60b1175c0d5d39bd261e0e25a3b054b640c841881d8ca46b198715edb050550",
    "wmap|rows1x7": "7bd18d5f3cd36c5d5fbf7820916408e6adefe4c11ca09255fbb85e3056e070a4",
    "wmap|rows64": "07e626e97b498d244534984db4fe0a7e62c8ac8945428fc9df791350ef153d93",
    "wmap|one": "41acc7d43dbeae95a3bc3c472e9adac1e1cd8d3a82a0231fc9042485c868d1bc",
    "wmap|diagonal": "0593781d3939e885199040e87188d6c79155d893ecc6dc736fc95d9545aa3f92",
    "wmap|islands": "9217fd2bedc2820dac7ee5d87ac47294a10090197f8821578f41c22882d4db00",
    "wmap|each16x12": "242c01239ff68f55a7570527937ffaf50a8dc6f8febeadb302db96949acd1560",
    "wmap|noise64x48": "54f57bfb695831e0c7d35b17c35dbe04fa6ad03eb7bae324b49c21bc12326ef1",
    "wmap|big": "c3f87dcc054a7be1543ca888f07472a3fc46557739dd8b12407dd999b7618220",
    "wmap|noise97x41-permuted": "6cf54e013abaa6f613bcea05aeb977b7573bfd17903ced18f3654840fcb124f1",
    "wmap|noise96x80": "3d5b110fc2f8336b5d0e41f07ff3fa42e831baca6be77458cc83f05fef37e4fb",
    "wmap|noise96x80-permuted": "bacbdad6e767cb3f3df8b51aad0406d803ba417f931541a7c0a92d05b3574808",
    "wmap|refused": "55f02b05db78238f43f173c429e9b56cdd4c0c38d6dc18061132851cf4266119",
    "wmap|noise512x300": "dd2e904bde6ac561d67fb090cde6d8e73ca92f69109140fdc41852aea72bd90f",
    "cases": "b90ac77fb4162d6d2626d03ee680f4791c1b86f3bd8e08ff0f013e4a29a9d484",
    "mask|random|48|64": "9e52b7c692c8da85011c4fccd13092907fe14f61c1d0cd6deb377c5a52c35833",
    "mask|block|48|64": "508ba2c6f0cf12a3c30b4c1d934bf85a7fc607bf61174895414aaab8ff1c2af3",
    "mask|island-window|48|64": "20f011d57b7b9aaf9f792a80995d04951357864638ad7aa3b57c6122df97070b",
    "mask|random|41|97": "82eb7d36701f8df5d3eba4adb7e7a4a98e1fca8620db3505e0385485a06d0d3c",
    "mask|block|41|97": "396c00372c1d69479df5e2757e27076446da846f405b3ff10a827a8403275edf",
    "tie|1|0|2": "fab844c7de9f534269b0bf0060b530ceb8c3fdaae7a7867893f0b0bb4ed19122",
    "tie|2|0|1": "e2eef7e107ec45c85d78c8e7fd9c64c479917427b07e3689eef172e2d13e20c0",
    "atsize|A": "a541633a16874f39b7730c0cd5c6052e30e2b0e21c7f24add4f4a2367eb618b2",
    "atsize|B": "97d77217f0fab143ebeb8ddd814bcc768c568fc1c0ed5bcc89e49bb7f3084cc4",
}


def digest(a, *extra):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(a.dtype.str.encode())
    h.update(repr(tuple(a.shape)).encode())
    h.update(a.tobytes())
    if extra:
        h.update(repr(extra).encode())
    return h.hexdigest()


def _ints(args):
    return [int(a) for a in args]


def _merge(name, field):
    i = ri.merge_inputs(name)
    return digest(i[field], i["w"], i["h"], i["connectivity"], i["R"])


BUILD = {
    "frame": lambda w, h: digest(ri.frame(int(w), int(h))),
    "noise": lambda w, h, k, seed, dtype: digest(ri.noise(int(w), int(h), int(k), seed=int(seed),
                                                          dtype=np.dtype(dtype).type)),
    "regions": lambda name, w, h: digest(ri.regions_base(name, int(w), int(h))),
    "widen": lambda name, w, h, width: digest(ri.widen(ri.regions_base(name, int(w), int(h)), int(width))),
    "adjacency": lambda name, w, h: digest(ri.adjacency_base(name, int(w), int(h))),
    "merge": _merge,
    "pixels": lambda name: digest(*ri.pixels_map(name)),
    "gaps": lambda *gaps: digest(*ri.with_gaps(ri.pixels_map("noise64x48")[0], *_ints(gaps))),
    "permuted": lambda name, seed: digest(ri.permuted(ri.pixels_map(name)[0], int(seed))),
    "relabel": lambda name: digest(ri.relabel_by_first(ri.pixels_map(name)[0][::-1])),
    "wmap": lambda name: digest(*ri.wmap(name)),
    "mask": lambda kind, h, w: digest(ri.mask_of(kind, int(h), int(w))),
    "tie": lambda *order: digest(*ri.tie_map(tuple(_ints(order)))),
    "atsize": lambda name: digest(atsize.labels(name)),
    "cases": lambda: hashlib.sha256(repr(ri.CASES).encode()).hexdigest(),
}


def test_every_kind_is_pinned():
    assert {key.split("|")[0] for key in PINNED} == set(BUILD)


@pytest.mark.parametrize("kind", sorted(BUILD))
def test_inputs_are_what_they_were(kind):
    for key, want in PINNED.items():
        head, *args = key.split("|")
        if head == kind:
            assert BUILD[kind](*args) == want, key


def test_the_cases_name_pinned_maps_and_no_mask_is_no_mask():
    assert {"wmap|%s" % name for name, _, _ in ri.CASES} <= set(PINNED)
    assert ri.mask_of(None, 3, 3) is None
